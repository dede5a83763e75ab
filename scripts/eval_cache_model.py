"""Developer: how often does the line search evaluate the same parameter FLOATS twice, and what would a launch gain if those
evaluations were free?  CPU only (EXPERIMENTS.md E69: the reasoning behind the memo of evaluations in gpsat_kernels.hip).

Part 1, emulation.  The bench's tiles (synthetic.make_tile, seeds t, N = 500, D = 3, RBF, default_bounds, theta0 = 1); the
objective and its gradient in numpy float32 with fp64 reductions, as the device forms them; the driver is SciPy's L-BFGS-B
(maxiter 20, ftol 1e-6, gtol 1e-5, maxls 20, maxcor 10) in the kernels' u-space.  Every evaluation's key -- the D + 2 floats
the device's evaluate() reads: (float)(1 / l_d), (float) sf2, (float) sn2 -- and its iteration are recorded.  This is an
emulation, not the device: SciPy's driver is not the on-device one, and the fp32 rounding differs.

Part 2, launch model.  T / 8 workgroups in CU pairs serve the tiles from a FIFO ring in slices of 4 computed evaluations; an
evaluation without a running CU-mate takes 0.77 of the time; a tile that finishes while others wait leaves its prediction to
workgroups on CUs where no fit runs.  Run with the trajectories as they are, and with repeated keys free.

    python scripts/eval_cache_model.py [--tiles 512] [--workers 16]
"""
import argparse
import heapq
import os
import sys
from collections import deque

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpsat_amd import synthetic as syn  # noqa: E402

N, D = 500, 3
HI_L = np.array([12.0, 12.0, 9.0])
LO_L = 1e-8
SHIFT = np.array([0.0, 1e-6])          # softplus shift of sf2, sn2 (gpsat_opt.h opt_fresh_tile)


def theta_of_u(u):
    th = np.empty(D + 2)
    th[:D] = LO_L + (HI_L - LO_L) / (1.0 + np.exp(-u[:D]))
    th[D:] = np.log1p(np.exp(-np.abs(u[D:]))) + np.maximum(u[D:], 0.0) + SHIFT
    return th


def u_of_theta(th):
    u = np.empty(D + 2)
    t = np.clip((th[:D] - LO_L) / (HI_L - LO_L), 1e-15, 1 - 1e-15)
    u[:D] = np.log(t / (1 - t))
    y = th[D:] - SHIFT
    u[D:] = np.log(-np.expm1(-y)) + y
    return u


def dtheta_du(th):
    d = np.empty(D + 2)
    d[:D] = (th[:D] - LO_L) * (HI_L - th[:D]) / (HI_L - LO_L)
    d[D:] = -np.expm1(-(th[D:] - SHIFT))
    return d


def key_of(th):
    return np.concatenate([(1.0 / th[:D]).astype(np.float32), th[D:].astype(np.float32)])


def nll_grad32(X, y, th):
    """float32 matrices, fp64 reductions; dNLL/dtheta at the fp64 theta"""
    k = key_of(th)
    invl, sf2, sn2 = k[:D], k[D], k[D + 1]
    Xs = X * invl
    d2 = [(Xs[:, None, d] - Xs[None, :, d]) ** 2 for d in range(D)]
    kf = np.exp(np.float32(-0.5) * (d2[0] + d2[1] + d2[2]))
    K = sf2 * kf + sn2 * np.eye(N, dtype=np.float32)
    try:
        L = np.linalg.cholesky(K)
    except np.linalg.LinAlgError:
        return np.inf, np.zeros(D + 2)
    Li = np.linalg.inv(L)
    z = Li @ y
    Kinv = Li.T @ Li
    alpha = Li.T @ z
    nll = 0.5 * float(np.sum(z.astype(np.float64) ** 2)) + float(np.sum(np.log(np.diag(L).astype(np.float64)))) \
        + 0.5 * N * 1.8378770664093453
    M = Kinv - np.outer(alpha, alpha)
    g = np.empty(D + 2)
    Mk = M * kf
    for d in range(D):
        g[d] = 0.5 * float(sf2) * float(np.sum((Mk * d2[d]).astype(np.float64))) / th[d]
    g[D] = 0.5 * float(np.sum(Mk.astype(np.float64)))
    g[D + 1] = 0.5 * float(np.trace(M.astype(np.float64)))
    if not np.isfinite(nll):
        return np.inf, np.zeros(D + 2)
    return nll, g


def run_tile(t):
    """-> list of (iteration, key bytes) of every evaluation of tile t"""
    from scipy.optimize import minimize
    X, y, _, _ = syn.make_tile(t, N, 0, D, 0)
    X, y = X.astype(np.float32), y.astype(np.float32)
    trace, it = [], [0]

    def fun(u):
        th = theta_of_u(u)
        f, g = nll_grad32(X, y, th)
        trace.append((it[0], key_of(th).tobytes()))
        return f, g * dtheta_du(th)

    def cb(_):
        it[0] += 1

    minimize(fun, u_of_theta(np.ones(D + 2)), jac=True, method="L-BFGS-B", callback=cb,
             options=dict(maxiter=20, ftol=1e-6, gtol=1e-5, maxls=20, maxcor=10))
    return trace


def computed(trace, k_memo):
    """per evaluation: False if its key is one of the k_memo most recent distinct keys of the tile (k_memo = 0: no memo)"""
    recent, out = deque(maxlen=max(k_memo, 1)), []
    for _, key in trace:
        hit = k_memo > 0 and key in recent
        out.append(not hit)
        if not hit:
            recent.append(key)
    return out


def launch_model(tiles, slice_len=4, alone=0.77, pred=0.55):
    """tiles: per tile the list of `computed` flags.  Returns (makespan, idle share of the workgroups' time), in evaluation units."""
    T = len(tiles)
    W = max(2, (T // 8) & ~1)
    ring = deque((t, 0) for t in range(T))
    busy = [False] * W                       # runs a fit
    events = [(0.0, w) for w in range(W)]    # (time, workgroup) asks for work
    heapq.heapify(events)
    deferred, work, end = 0, 0.0, 0.0
    while events:
        now, w = heapq.heappop(events)
        busy[w] = False
        if ring:
            t, pos = ring.popleft()
            busy[w] = True
            flags, dt, n = tiles[t], 0.0, 0
            while pos < len(flags) and n < slice_len:
                if flags[pos]:
                    dt += 1.0 if busy[w ^ 1] else alone
                    n += 1
                pos += 1
            while pos < len(flags) and not flags[pos]:
                pos += 1                     # answered evaluations cost nothing and take no slice
            if pos < len(flags):
                ring.append((t, pos))
            elif ring:
                deferred += 1                # others wait: the prediction is left for the end
            else:
                dt += pred if busy[w ^ 1] else pred * alone
            work += dt
            end = max(end, now + dt)
            heapq.heappush(events, (now + dt, w))
        elif deferred > 0 and not busy[w ^ 1]:
            deferred -= 1
            work += pred * alone
            end = max(end, now + pred * alone)
            heapq.heappush(events, (now + pred * alone, w))
        elif deferred > 0 or any(busy):
            heapq.heappush(events, (now + 0.25, w))      # a fit still runs somewhere: look again later
    return end, 1.0 - work / (W * end)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=512)
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--memo", type=int, default=4, help="distinct keys kept per tile")
    a = ap.parse_args()
    from multiprocessing import get_context
    from threadpoolctl import threadpool_limits
    with threadpool_limits(1):
        if a.workers > 1:
            with get_context("fork").Pool(a.workers) as pool:
                traces = pool.map(run_tile, range(a.tiles), chunksize=4)
        else:
            traces = [run_tile(t) for t in range(a.tiles)]
    n = np.array([len(tr) for tr in traces])
    iters = np.array([tr[-1][0] for tr in traces])
    print(f"{a.tiles} tiles: {n.mean():.2f} evaluations per tile (max {n.max()}), {iters.mean():.2f} iterations; "
          f"tiles with >= 30 evaluations {100 * (n >= 30).mean():.1f} %")
    flags = [computed(tr, a.memo) for tr in traces]
    rep = np.array([len(f) - sum(f) for f in flags])
    prev = sum(sum(1 for i in range(1, len(tr)) if tr[i][1] == tr[i - 1][1]) for tr in traces)
    long_t = n >= 36
    print(f"repeated keys (memo of {a.memo}): {rep.sum()} of {n.sum()} evaluations ({100 * rep.sum() / n.sum():.2f} %), "
          f"{prev} repeat the evaluation just before; in {(rep > 0).sum()} tiles; the {long_t.sum()} tiles with >= 36 evaluations "
          f"hold {rep[long_t].sum()}; longest tile {n.max()} -> {(n - rep).max()} computed evaluations")
    pos_in_search = []
    for tr, f in zip(traces, flags):
        start = 0
        for i in range(len(tr)):
            if i and tr[i][0] != tr[i - 1][0]:
                start = i
            if not f[i]:
                pos_in_search.append(i - start + 1)
    if pos_in_search:
        print(f"earliest repeat inside an iteration's evaluations: number {min(pos_in_search)}")
    base = launch_model([[True] * len(f) for f in flags])
    memo = launch_model(flags)
    print(f"launch model, FIFO ring, slices of 4: makespan {base[0]:.1f} (idle {100 * base[1]:.1f} %) -> {memo[0]:.1f} "
          f"(idle {100 * memo[1]:.1f} %) with repeats free: {100 * (memo[0] / base[0] - 1):+.1f} %")


if __name__ == "__main__":
    main()
