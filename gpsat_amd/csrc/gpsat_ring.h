// gpsat_ring.h -- the time-sliced tile queue of the persistent tile kernels (device side), shared by the fp32 and fp64 kernels.
#ifndef GPSAT_RING_H
#define GPSAT_RING_H
#include <hip/hip_runtime.h>
#include "gpsat_kernels.h"

namespace gpsat {

// ---------------------------------------------------------------------------------------------
// time slicing (KernelArgs::seg_cost > 0): the tiles circulate through a ring in device memory.  An entry is
// (sequence + 1) << 32 | resumed << 31 | tile; slot s lives at s & ring_mask.  The ring is larger than the number of tiles
// plus the number of workgroups, so a slot is never rewritten before the workgroup that claimed it has read it.
// One thread per workgroup calls these.
// ---------------------------------------------------------------------------------------------
static __device__ __forceinline__ int ring_pop(const KernelArgs& A) {
    const unsigned s = (unsigned)__hip_atomic_fetch_add(&A.ring_ctl[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long* e = A.ring + (s & (unsigned)A.ring_mask);
    for (int spins = 0;; ++spins) {
        // relaxed sc1 polling, no acquire fence anywhere: a resumed tile's state is read with sc1 loads only (they bypass
        // this CU's L1), after the workgroup barrier that follows this poll (gp_tile_kernel)
        const unsigned long long v = __hip_atomic_load(e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)(v >> 32) == s + 1u) return (int)(unsigned)v;
        // nothing there yet: either a tile will be pushed back, or every tile is finished
        if (__hip_atomic_load(&A.ring_ctl[32], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= 0) return -1;
        // never reached by design (minutes of polling): a lost entry must not hang the GPU; the host sees unfinished tiles
        if (spins > (1 << 25)) return -1;
        __builtin_amdgcn_s_sleep(64);
    }
}

// The two halves of ring_pop for a workgroup that does something else while its slot is empty (cooperative tiles: it
// helps a running tile): claim a slot once, then look at it.  ring_look: the entry, -1 when every tile is finished,
// -2 when the slot is still empty.
static __device__ __forceinline__ unsigned ring_claim(const KernelArgs& A) {
    return (unsigned)__hip_atomic_fetch_add(&A.ring_ctl[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static __device__ __forceinline__ int ring_look(const KernelArgs& A, unsigned s) {
    const unsigned long long v = __hip_atomic_load(A.ring + (s & (unsigned)A.ring_mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((unsigned)(v >> 32) == s + 1u) return (int)(unsigned)v;
    if (__hip_atomic_load(&A.ring_ctl[32], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= 0) return -1;
    return -2;
}

// entries pushed and not yet claimed (<= 0: whoever pops next waits): a tile that would be suspended now would only move to
// a workgroup that is waiting for it -- it may as well keep running where it is
static __device__ __forceinline__ int ring_waiting_tiles(const KernelArgs& A) {
    return __hip_atomic_load(&A.ring_ctl[16], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) -
           __hip_atomic_load(&A.ring_ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static __device__ __forceinline__ void ring_push(const KernelArgs& A, int tile) {
    const unsigned s = (unsigned)__hip_atomic_fetch_add(&A.ring_ctl[16], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long v = ((unsigned long long)(s + 1u) << 32) | 0x80000000ull | (unsigned)tile;
    __hip_atomic_store(A.ring + (s & (unsigned)A.ring_mask), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------
// deferred predictions (KernelArgs::pq): snapshot slot s is taken once per launch (no reuse: the predictions run at the end
// of the launch, when no fit is left to defer), its entry published after the snapshot's stores have drained.  A slot number
// past pq_slots means the pool is full: the tile predicts inline.  One thread per workgroup calls these.
// ---------------------------------------------------------------------------------------------
static __device__ __forceinline__ int pq_take_slot(const KernelArgs& A) {
    const int s = __hip_atomic_fetch_add(&A.pq_ctl[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return s < A.pq_slots ? s : -1;
}

static __device__ __forceinline__ void pq_publish(const KernelArgs& A, int s, int tile) {
    __hip_atomic_store(&A.pq[s], (unsigned long long)tile + 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the next taken slot, -1 when every taken slot is claimed already
static __device__ __forceinline__ int pq_claim(const KernelArgs& A) {
    int c = __hip_atomic_load(&A.pq_ctl[16], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int n = min(__hip_atomic_load(&A.pq_ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), A.pq_slots);
    while (c < n)
        if (__hip_atomic_compare_exchange_strong(&A.pq_ctl[16], &c, c + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return c;
    return -1;
}

// the tile of a claimed slot: its owner publishes it once the snapshot is written (microseconds).  -1 only after minutes
// (never by design): the tile stays unfinished, the ring's waits give up, and the host sees unfinished tiles.
static __device__ __forceinline__ int pq_wait_entry(const KernelArgs& A, int s) {
    for (int spins = 0;; ++spins) {
        const unsigned long long v = __hip_atomic_load(&A.pq[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v) return (int)(v - 1ull);
        if (spins > (1 << 25)) return -1;
        __builtin_amdgcn_s_sleep(64);
    }
}

// this workgroup's CU: XCC_ID << 8 | HW_ID[15:8] (SE, SH, CU), < 2048 (KernelArgs::cu_busy)
static __device__ __forceinline__ int cu_index() {
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20) & 7;
    return (int)((xcc << 8) | ((hw >> 8) & 0xff));
}

}  // namespace gpsat
#endif
