// gpsat_key_runs.hip -- the keyed sort-and-run-heads stage on gfx950: rows with a 64-bit key each, grouped on the device.
// Its users are the binning (gpsat_bin.hip), the keyed glues (gpsat_post.hip) and the grouped tracks (gpsat_prep.hip through
// the glue's keys); DESIGN.md section 26 is its contract.
//
// The caller has written keys[i] and rows[i] = i (its key kernel); rows that take no part carry k.sentinel, which is above
// every other key.  key_runs then (1) sorts (key, source row) with rocPRIM's STABLE radix sort over the bits of the sentinel,
// so the rows of a key stay in source order in perm[]; (2) has the head flag of every run of equal keys written, by the
// caller's step when it gives one (binning gathers its values in the same pass) and by key_runs_flag_kernel otherwise;
// (3) selects the run starts; (4) drops the sentinel's run, which is the last when there is one: counts[0] = n runs kept,
// counts[1] = starts[n] = rows in them.  Everything stays on the device and in the stream: the caller reads counts.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include "gpsat_kernels.h"

namespace gpsat {

__global__ void __launch_bounds__(256) key_runs_flag_kernel(const KeyRuns k) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= k.R) return;
    k.flags[i] = key_run_head(k.keys_sorted, i);
}

// runs -> groups: the sentinel's run, when there is one, is the last; starts[n] = first row past the groups
__global__ void key_runs_finish_kernel(const KeyRuns k) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    long long n = *k.n_runs;
    long long valid = k.R;
    if (n > 0 && k.keys_sorted[k.starts[n - 1]] == k.sentinel) { valid = k.starts[n - 1]; --n; }
    k.starts[n] = (unsigned)valid;
    k.counts[0] = n;
    k.counts[1] = valid;
}

static inline int key_bits(unsigned long long sentinel) {
    int bits = 1;
    while (bits < 64 && (sentinel >> bits) != 0) ++bits;
    return bits;
}

hipError_t key_runs(const KeyRuns& k, KeyRunsFlags* write_flags, const void* ctx, hipEvent_t after_sort, void* temp,
                    size_t& temp_bytes, hipStream_t stream) {
    const int bits = key_bits(k.sentinel);
    rocprim::counting_iterator<unsigned> rows0(0);
    if (!temp) {
        size_t t1 = 0, t2 = 0;
        hipError_t e = rocprim::radix_sort_pairs(nullptr, t1, k.keys, k.keys_sorted, k.rows, k.perm, (size_t)k.R, 0, bits, stream);
        if (e != hipSuccess) return e;
        e = rocprim::select(nullptr, t2, rows0, k.flags, k.starts, k.n_runs, (size_t)k.R, stream);
        temp_bytes = t1 > t2 ? t1 : t2;
        return e;
    }
    hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, k.keys, k.keys_sorted, k.rows, k.perm, (size_t)k.R, 0, bits, stream);   // stable
    if (e != hipSuccess) return e;
    if (after_sort && (e = hipEventRecord(after_sort, stream)) != hipSuccess) return e;
    if (write_flags) write_flags(ctx, stream);
    else hipLaunchKernelGGL(key_runs_flag_kernel, dim3((unsigned)((k.R + 255) / 256)), dim3(256), 0, stream, k);
    e = rocprim::select(temp, temp_bytes, rows0, k.flags, k.starts, k.n_runs, (size_t)k.R, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(key_runs_finish_kernel, dim3(1), dim3(64), 0, stream, k);
    return hipGetLastError();
}

}  // namespace gpsat
