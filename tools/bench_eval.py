#!/usr/bin/env python
"""Device time of mpcb_eval with and without res_stat, next to mpcb_linearize at the same shape.

mpcb_linearize integrates the same 16 RK4 tangents per stage as the adjoint sweep of mpcb_eval and
also stores [A|B] (1.5 KB per stage in fp64), so it is the yardstick.  Shapes: c2 (4096 x N = 20,
fp64) and c3 (65536 x N = 20, fp32).  HIP events around ``--inner`` back-to-back calls, median of
``--runs`` after ``--warmup`` calls of every variant, the variants alternating so drift hits them
alike.  Prints one JSON line per shape.

    python tools/bench_eval.py [--runs 20] [--warmup 5] [--inner 10]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench(name, B, N, dtype, runs, warmup, inner):
    import torch

    from mpc_blaster_amd import BatchedMPC, MPCConfig, _lib
    m = BatchedMPC(MPCConfig(N=N, dtype=dtype), max_batch=B)
    inp = m.gen_inputs(B, seed=1003, ref='sine', wind=False)
    m.solve(inp['x0'], inp['xref'], inp['uref'])           # an iterate worth evaluating: one RTI step
    X, U = m.get_state_trajectory().clone(), m.get_input_trajectory().clone()
    # the C ABI directly on preallocated arrays, ``inner`` launches per event pair: the events then
    # time the device, not the host's path to the launch
    lib, h, P, null, st = m.lib, m._h, m._ptr, m._ptr(None), m._stream()
    A = torch.empty((B, N, 12, 12), dtype=X.dtype, device=X.device)
    Bm = torch.empty((B, N, 12, 4), dtype=X.dtype, device=X.device)
    xn = torch.empty((B, N, 12), dtype=X.dtype, device=X.device)
    o = [torch.empty((B,), dtype=X.dtype, device=X.device) for _ in range(4)]
    xr, ur, x0 = inp['xref'], inp['uref'], inp['x0']
    xr_sb = (N + 1) * 12

    def ev_call(stat):
        return lambda: _lib.check(lib.mpcb_eval(h, B, P(x0), 12, P(X), P(U), P(xr), xr_sb, P(ur), 0, null, 0,
                                                P(o[0]), P(o[1]), P(o[2]), P(o[3]) if stat else null, st))
    variants = {
        'linearize': lambda: _lib.check(lib.mpcb_linearize(h, B, P(X), P(U), null, 0, P(A), P(Bm), P(xn), st)),
        'eval_stat': ev_call(True),
        'eval_nostat': ev_call(False),
    }
    for _ in range(warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(runs):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(inner):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / inner)
    ev = {k: v.cpu().numpy() for k, v in m.evaluate(X, U, xr, ur, x0=x0).items()}
    out = dict(shape=name, B=B, N=N, dtype=dtype, runs=runs, inner=inner,
               **{f'{k}_ms': round(statistics.median(v), 4) for k, v in ms.items()},
               **{f'{k}_min_ms': round(min(v), 4) for k, v in ms.items()},
               res_eq_max=float(np.nanmax(ev['res_eq'])), res_stat_max=float(np.nanmax(ev['res_stat'])))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--inner', type=int, default=10, help='launches per event pair')
    a = ap.parse_args()
    bench('c2', 4096, 20, 'f64', a.runs, a.warmup, a.inner)
    bench('c3', 65536, 20, 'f32', a.runs, a.warmup, a.inner)


if __name__ == '__main__':
    main()
