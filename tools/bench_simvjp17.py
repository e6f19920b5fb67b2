#!/usr/bin/env python
"""Device time of mpcb_sim_step_vjp17 (the reverse mode of the 17/6 plant step) next to the forward
kernel it differentiates and to the forward-mode route to the same gx, gu.

Variants, all on one 17/6 handle of N = 1 with a parameter vector per instance:
  sim_step      mpcb_sim_step_p17, the plant step itself
  vjp_xu        mpcb_sim_step_vjp17 with gx and gu only
  vjp_all       ... with gx, gu and gparams
  linearize     mpcb_linearize: [A | B] of the same step written to memory (B x 17 x 23 values), 16
                tangent lanes per instance; the products A^T g, B^T g would still have to follow

Shapes: B = 4096 and 65536 in fp64 and fp32; x in U(-0.5, 0.5), motor inputs in U(0, 65), swivel rates
in U(-0.087, 0.087), p[:24] ~ 0.3 N(0, 1), T_blast in U(10, 30), gxn ~ N(0, 1), all drawn on the device.
HIP events around ``--inner`` back-to-back calls, median of ``--runs`` after ``--warmup`` calls of
every variant, the variants alternating so drift hits them alike (the rules of tools/bench_simvjp.py).
Before timing, gx and gu of vjp_xu are compared with A^T g, B^T g of the linearize variant.  Prints
one JSON line per (dtype, B).

    python tools/bench_simvjp17.py [--batches 4096 65536] [--runs 20] [--warmup 5] [--inner 50]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench(dtype, B, runs, warmup, inner):
    import torch

    from mpc_blaster_amd import BatchedMPC, MPCConfig, _lib
    m = BatchedMPC(MPCConfig.full(N=1, dtype=dtype), max_batch=B)
    dev, dt = m._tdev, m.dtype
    gen = torch.Generator(device=dev).manual_seed(1017)

    def uni(lo, hi, *shape):
        return lo + (hi - lo) * torch.rand(shape, dtype=dt, device=dev, generator=gen)
    x = uni(-0.5, 0.5, B, 17)
    u = torch.cat([uni(0.0, 65.0, B, 4), uni(-0.087, 0.087, B, 2)], dim=1).contiguous()
    p = torch.cat([0.3 * torch.randn((B, 24), dtype=dt, device=dev, generator=gen), uni(10.0, 30.0, B, 1)],
                  dim=1).contiguous()
    g = torch.randn((B, 17), dtype=dt, device=dev, generator=gen)
    m.set_params(p)   # mpcb_linearize reads the handle's parameters
    xbar = torch.stack([x, x], dim=1).contiguous()
    new = lambda *s: torch.empty(s, dtype=dt, device=dev)   # noqa: E731
    xo, gx, gu, gp = new(B, 17), new(B, 17), new(B, 6), new(B, 25)
    A, Bm, xn = new(B, 1, 17, 17), new(B, 1, 17, 6), new(B, 1, 17)
    P, null, st, T = m._ptr, m._ptr(None), m._stream(), float(m.cfg.dt)

    def vjp(all3):
        return lambda: _lib.check(m.lib.mpcb_sim_step_vjp17(m._h, B, P(x), P(u), P(p), 25, T, P(g), P(gx), P(gu),
                                                            P(gp) if all3 else null, st))
    variants = {
        'sim_step': lambda: _lib.check(m.lib.mpcb_sim_step_p17(m._h, B, P(x), P(u), P(p), 25, T, P(xo), st)),
        'vjp_xu': vjp(False), 'vjp_all': vjp(True),
        'linearize': lambda: _lib.check(m.lib.mpcb_linearize(m._h, B, P(xbar), P(u), null, 0, P(A), P(Bm), P(xn), st)),
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
               **{f'{k}_over_sim_step': round(med[k] / med['sim_step'], 3) for k in med if k.startswith('vjp')},
               **{f'{k}_over_linearize': round(med[k] / med['linearize'], 3) for k in med if k.startswith('vjp')},
               vjp_xu_against_linearize=agree, finite=bool(torch.isfinite(gp).all()))
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
