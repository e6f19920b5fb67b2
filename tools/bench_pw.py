#!/usr/bin/env python
"""Device time of mpcb_solve_iterate_pw (the RTI step with cost weights per instance) next to
mpcb_solve_iterate and mpcb_solve_vjp at the same shape, and of mpcb_solve_vjp_pw next to
mpcb_solve_vjp_w.

Without the box the per-instance solve runs the passes of mpcb_solve_vjp (nominal by stage owner,
backward Riccati, forward) plus the solve's linear terms and 304 weight loads per instance, so the
product's time in the same run is what to compare with; mpcb_solve_iterate is the handle's tuned
path.  ``pw_null`` is the same kernel with the three weight pointers NULL (the handle's matrices,
stride 0): the difference to ``pw`` is what the per-instance loads cost.

Shapes: c2 (4096 x N = 20, fp64, hover); with ``--box`` c4's (N = 30, hover, input box [0, 65]) in
fp64, ``--batch`` instances of it (default one 65536 shard).  The iterate is one rollout-mode RTI
step; the weights are the handle's under a random SPD congruence per instance (e = exp(0.35 N(0, 1)),
drawn on the device); U of the timed per-instance solve gives the products' active set.  HIP events
around ``--inner`` back-to-back calls, median of ``--runs`` after ``--warmup`` calls of every
variant, the variants alternating so drift hits them alike.  Prints one JSON line.

    python tools/bench_pw.py [--box] [--batch B] [--runs 20] [--warmup 5] [--inner 5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench(box, B, runs, warmup, inner):
    import numpy as np
    import torch

    from mpc_blaster_amd import BatchedMPC, MPCConfig, _lib
    N, seed = (30, 1004) if box else (20, 1002)
    m = BatchedMPC(MPCConfig(N=N, dtype='f64', lbu=np.zeros(4) if box else None,
                             ubu=np.full(4, 65.0) if box else None), max_batch=B)
    inp = m.gen_inputs(B, seed=seed, ref='hover', wind=False)
    m.solve(inp['x0'], inp['xref'], inp['uref'])
    xbar, ubar = m.get_state_trajectory().clone(), m.get_input_trajectory().clone()
    x0, xr, ur = inp['x0'], inp['xref'], inp['uref']
    dev, dt = xbar.device, xbar.dtype
    gen = torch.Generator(device=dev).manual_seed(seed)

    def congruent(W):
        W = torch.as_tensor(np.asarray(W, dtype=np.float64), device=dev)
        e = torch.exp(0.35 * torch.randn((B, W.shape[0]), dtype=dt, device=dev, generator=gen))
        return (W[None] * e[:, :, None] * e[:, None, :]).contiguous()
    Qw, Rw, QNw = congruent(m.cfg.Q), congruent(m.cfg.R), congruent(m.cfg.QN)
    gX = torch.randn((B, N + 1, 12), dtype=dt, device=dev, generator=gen)
    gU = torch.randn((B, N, 4), dtype=dt, device=dev, generator=gen)

    def outs():
        return (torch.empty((B, 4), dtype=dt, device=dev), torch.empty_like(xbar), torch.empty_like(ubar),
                torch.empty((B,), dtype=torch.int32, device=dev))
    o_s, o_pw, o_null = outs(), outs(), outs()
    gx0, gxr, gur = torch.empty((B, 12), dtype=dt, device=dev), torch.empty_like(xbar), torch.empty_like(ubar)
    gQ, gR = torch.empty((B, 12, 12), dtype=dt, device=dev), torch.empty((B, 4, 4), dtype=dt, device=dev)
    gQN = torch.empty_like(gQ)
    sts = {k: torch.empty((B,), dtype=torch.int32, device=dev) for k in ('vjp', 'vjp_w', 'vjp_pw')}
    P, null, st = m._ptr, m._ptr(None), m._stream()

    def pw_call(o, W):
        return lambda: _lib.check(m.lib.mpcb_solve_iterate_pw(
            m._h, B, P(x0), 12, P(xbar), P(ubar), P(xr), 0, P(ur), 0, null, 0, W[0], 144 if W[0] else 0, W[1],
            16 if W[1] else 0, W[2], 144 if W[2] else 0, P(o[0]), P(o[1]), P(o[2]), P(o[3]), st))
    Us = P(o_pw[2]) if box else null   # the products' active set: the per-instance solve's U
    variants = {
        'solve_iterate': lambda: _lib.check(m.lib.mpcb_solve_iterate(
            m._h, B, P(x0), 12, P(xbar), P(ubar), P(xr), 0, P(ur), 0, null, 0, P(o_s[0]), P(o_s[1]), P(o_s[2]),
            P(o_s[3]), st)),
        'pw': pw_call(o_pw, (P(Qw), P(Rw), P(QNw))),
        'pw_null': pw_call(o_null, (None, None, None)),
        'vjp': lambda: _lib.check(m.lib.mpcb_solve_vjp(m._h, B, P(xbar), P(ubar), Us, null, 0, P(gX), P(gU), P(gx0),
                                                       P(gxr), P(gur), P(sts['vjp']), st)),
        'vjp_w': lambda: _lib.check(m.lib.mpcb_solve_vjp_w(
            m._h, B, P(xbar), P(ubar), P(o_pw[1]), P(o_pw[2]), P(xr), 0, P(ur), 0, null, 0, P(gX), P(gU), P(gx0),
            P(gxr), P(gur), P(gQ), P(gR), P(gQN), P(sts['vjp_w']), st)),
        'vjp_pw': lambda: _lib.check(m.lib.mpcb_solve_vjp_pw(
            m._h, B, P(xbar), P(ubar), P(o_pw[1]), P(o_pw[2]), P(xr), 0, P(ur), 0, null, 0, P(Qw), 144, P(Rw), 16,
            P(QNw), 144, P(gX), P(gU), P(gx0), P(gxr), P(gur), P(gQ), P(gR), P(gQN), P(sts['vjp_pw']), st)),
    }
    for _ in range(warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(runs):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(inner):
                f()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1) / inner)
    med = {k: statistics.median(v) for k, v in t.items()}
    U = o_pw[2]
    out = dict(shape='c4-fp64' if box else 'c2', B=B, N=N, dtype='f64', box=box, runs=runs, inner=inner,
               **{f'{k}_ms': round(v, 4) for k, v in med.items()},
               **{f'{k}_min_ms': round(min(v), 4) for k, v in t.items()},
               pw_over_vjp=round(med['pw'] / med['vjp'], 3),
               pw_over_solve=round(med['pw'] / med['solve_iterate'], 3),
               pw_over_pw_null=round(med['pw'] / med['pw_null'], 3),
               vjp_pw_over_vjp_w=round(med['vjp_pw'] / med['vjp_w'], 3),
               solve_status_ok=int((o_s[3] == 0).sum()), pw_status_ok=int((o_pw[3] == 0).sum()),
               pw_status_maxiter=int((o_pw[3] == 2).sum()),
               **{f'{k}_status_ok': int((v == 0).sum()) for k, v in sts.items()},
               clamped_fraction=(float(((U <= 0.0) | (U >= 65.0)).double().mean()) if box else 0.0))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--box', action='store_true', help="c4's shape in fp64 (N = 30, input box [0, 65])")
    ap.add_argument('--batch', type=int, default=None, help='instances (default: 4096, with --box 65536)')
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--inner', type=int, default=5, help='launches per event pair')
    a = ap.parse_args()
    bench(a.box, a.batch or (65536 if a.box else 4096), a.runs, a.warmup, a.inner)


if __name__ == '__main__':
    main()
