#!/usr/bin/env python
"""Device time of mpcb_sim_step_vjp (the reverse mode of the plant step) next to the forward kernels
it differentiates and to the forward-mode route to the same gx, gu.

Variants, each on the handle's vehicle and with a vehicle record per instance (``_pm``):
  sim_step, sim_step_pm         the plant step itself
  vjp_xu, vjp_xu_pm             mpcb_sim_step_vjp with gx and gu only
  vjp_all, vjp_all_pm           ... with gx, gu, gwind and gmodel
  linearize                     mpcb_linearize on a handle of N = 1: [A | B] of the same step written
                                to memory (B x 12 x 16 values), 16 tangent lanes per instance; the
                                products A^T g, B^T g would still have to follow

Shapes: B = 4096 and 65536 in fp64 and fp32; x in U(-0.5, 0.5), u in U(0, 65), wind in U(-2, 2),
gxn ~ N(0, 1), the vehicles of tools/bench_pm.py, all drawn on the device.  HIP events around
``--inner`` back-to-back calls, median of ``--runs`` after ``--warmup`` calls of every variant, the
variants alternating so drift hits them alike.  Before timing, gx and gu of vjp_xu are compared
with A^T g, B^T g of the linearize variant.  Prints one JSON line per (dtype, B).

    python tools/bench_simvjp.py [--batches 4096 65536] [--runs 20] [--warmup 5] [--inner 50]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench(dtype, B, runs, warmup, inner):
    import numpy as np
    import torch

    from mpc_blaster_amd import BatchedMPC, MPCConfig, _lib
    m = BatchedMPC(MPCConfig(N=1, dtype=dtype), max_batch=B)
    dev, dt = m._tdev, m.dtype
    gen = torch.Generator(device=dev).manual_seed(1002)

    def uni(lo, hi, *shape):
        return lo + (hi - lo) * torch.rand(shape or (B,), dtype=dt, device=dev, generator=gen)

    def congruent(W, sigma):
        W = torch.as_tensor(np.asarray(W, dtype=np.float64), dtype=dt, device=dev)
        e = torch.exp(sigma * torch.randn((B, W.shape[0]), dtype=dt, device=dev, generator=gen))
        return (W[None] * e[:, :, None] * e[:, None, :]).contiguous()
    x, u, wind = uni(-0.5, 0.5, B, 12), uni(0.0, 65.0, B, 4), uni(-2.0, 2.0, B, 3)
    g = torch.randn((B, 12), dtype=dt, device=dev, generator=gen)
    model = m.pack_model(B, mass=m.cfg.mass * uni(0.8, 1.25), lx=m.cfg.lx * uni(0.9, 1.1), ly=m.cfg.ly * uni(0.9, 1.1),
                         c=m.cfg.c * uni(0.9, 1.1), t_blast=uni(0.0, 5.0), J=congruent(m.cfg.J, 0.2))
    xbar = torch.stack([x, x], dim=1).contiguous()
    new = lambda *s: torch.empty(s, dtype=dt, device=dev)   # noqa: E731
    xo, gx, gu, gw, gm = new(B, 12), new(B, 12), new(B, 4), new(B, 3), new(B, 14)
    A, Bm, xn = new(B, 1, 12, 12), new(B, 1, 12, 4), new(B, 1, 12)
    P, null, st, T = m._ptr, m._ptr(None), m._stream(), float(m.cfg.dt)

    def vjp(md, all4):
        return lambda: _lib.check(m.lib.mpcb_sim_step_vjp(
            m._h, B, P(x), P(u), P(wind), 3, P(md), 14 if md is not None else 0, T, P(g), P(gx), P(gu),
            P(gw) if all4 else null, P(gm) if all4 else null, st))
    variants = {
        'sim_step': lambda: _lib.check(m.lib.mpcb_sim_step(m._h, B, P(x), P(u), P(wind), 3, T, P(xo), st)),
        'sim_step_pm': lambda: _lib.check(m.lib.mpcb_sim_step_pm(m._h, B, P(x), P(u), P(wind), 3, P(model), 14, T,
                                                                 P(xo), st)),
        'vjp_xu': vjp(None, False), 'vjp_xu_pm': vjp(model, False),
        'vjp_all': vjp(None, True), 'vjp_all_pm': vjp(model, True),
        'linearize': lambda: _lib.check(m.lib.mpcb_linearize(m._h, B, P(xbar), P(u), P(wind), 3, P(A), P(Bm), P(xn),
                                                             st)),
    }
    # the two routes give the same gx, gu
    variants['linearize']()
    variants['vjp_xu']()
    torch.cuda.synchronize()
    agree = max(float((torch.einsum('bij,bi->bj', M[:, 0], g) - v).abs().max() / v.abs().max())
                for M, v in ((A, gx), (Bm, gu)))
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
            t[k].append(e0.elapsed_time(e1) / inner * 1e3)
    med = {k: statistics.median(v) for k, v in t.items()}
    out = dict(B=B, dtype=dtype, runs=runs, inner=inner,
               **{f'{k}_us': round(v, 2) for k, v in med.items()},
               **{f'{k}_min_us': round(min(v), 2) for k, v in t.items()},
               **{f'{k}_over_sim_step_pm': round(med[k] / med['sim_step_pm'], 3) for k in med if k.startswith('vjp')},
               vjp_xu_over_linearize=round(med['vjp_xu'] / med['linearize'], 3),
               vjp_xu_against_linearize=agree, finite=bool(torch.isfinite(gm).all() and torch.isfinite(gw).all()))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[4096, 65536], help='instances')
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--inner', type=int, default=50, help='launches per event pair')
    a = ap.parse_args()
    for dtype in ('f64', 'f32'):
        for B in a.batches:
            bench(dtype, B, a.runs, a.warmup, a.inner)


if __name__ == '__main__':
    main()
