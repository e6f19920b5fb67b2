#!/usr/bin/env python
"""Device time of mpcb_solve_gains next to mpcb_solve_iterate and next to the vector-Jacobian
product asked for gx0 only (mpcb_solve_vjp / mpcb_solve_vjp17 with gxref = guref = NULL), which
runs the same two passes: the nominal / linearisation pass and one backward Riccati sweep.  The
gains call does a subset of the product's arithmetic per stage (no linear term) and adds the
N * nu * nx stores of K per instance.

Method of tools/bench_vjp.py: the iterate is one rollout-mode RTI step; HIP events around
``--inner`` back-to-back C-ABI calls, median of ``--runs`` after ``--warmup`` calls of every
variant, the variants alternating so drift hits them alike.  The whole measurement is repeated
``--repeats`` times and every median is printed, so the spread between repeated medians stands
next to the difference between variants.  Shapes: c2 (4096 x N = 20, fp64) and c3 (65536 x
N = 20, fp32); ``--full17`` the 17/6 model at 4096 x N = 60, fp64 (the draws of
tools/bench_full17.py), with an empty and a half-full mask.  Prints one JSON line per shape.

    python tools/bench_gains.py [--runs 10] [--warmup 3] [--inner 3] [--repeats 3] [--rotate 0] [--shapes c2,c3] [--full17]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    # name: (B, N, dtype, references, seed)
    'c2': (4096, 20, 'f64', 'hover', 1002),
    'c3': (65536, 20, 'f32', 'sine', 1003),
}


def _time(variants, runs, warmup, inner, repeats, rotate=0):
    """{variant: [median ms of each repeat]}, {variant: min ms over everything}"""
    import torch
    keys = list(variants)
    variants = {k: variants[k] for k in keys[rotate % len(keys):] + keys[:rotate % len(keys)]}
    for _ in range(warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    meds, mins = {k: [] for k in variants}, {k: float('inf') for k in variants}
    for _ in range(repeats):
        t = {k: [] for k in variants}
        for _r in range(runs):
            for k, f in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _i in range(inner):
                    f()
                e1.record()
                e1.synchronize()
                t[k].append(e0.elapsed_time(e1) / inner)
        for k, v in t.items():
            meds[k].append(statistics.median(v))
            mins[k] = min(mins[k], min(v))
    return meds, mins


def _report(out, meds, mins, base):
    mid = {k: statistics.median(v) for k, v in meds.items()}
    out.update({f'{k}_ms': [round(x, 4) for x in v] for k, v in meds.items()})
    out.update({f'{k}_min_ms': round(v, 4) for k, v in mins.items()})
    out.update({f'{k}_spread_ms': round(max(v) - min(v), 4) for k, v in meds.items()})
    out.update({f'{k}_over_{base}': round(mid[k] / mid[base], 3) for k in mid if k.startswith('gains')})
    out.update({f'{k}_over_solve': round(mid[k] / mid['solve_iterate'], 3) for k in mid if k != 'solve_iterate'})
    print(json.dumps(out), flush=True)
    return out


def bench(name, runs, warmup, inner, repeats, rotate=0):
    import torch

    from mpc_blaster_amd import BatchedMPC, MPCConfig, _lib
    B, N, dtype, ref, seed = SHAPES[name]
    m = BatchedMPC(MPCConfig(N=N, dtype=dtype), max_batch=B)
    inp = m.gen_inputs(B, seed=seed, ref=ref, wind=False)
    m.solve(inp['x0'], inp['xref'], inp['uref'])
    xbar, ubar = m.get_state_trajectory().clone(), m.get_input_trajectory().clone()
    x0, xr, ur = inp['x0'], inp['xref'], inp['uref']
    xr_sb = (N + 1) * 12 if ref == 'sine' else 0
    dev, dt = xbar.device, xbar.dtype
    gen = torch.Generator(device=dev).manual_seed(seed)
    gX = torch.randn((B, N + 1, 12), dtype=dt, device=dev, generator=gen)
    gU = torch.randn((B, N, 4), dtype=dt, device=dev, generator=gen)
    u0 = torch.empty((B, 4), dtype=dt, device=dev)
    X, U = torch.empty_like(xbar), torch.empty_like(ubar)
    gx0 = torch.empty((B, 12), dtype=dt, device=dev)
    K = torch.empty((B, N, 4, 12), dtype=dt, device=dev)
    P0 = torch.empty((B, 12, 12), dtype=dt, device=dev)
    sts = {k: torch.empty((B,), dtype=torch.int32, device=dev) for k in ('solve_iterate', 'vjp_gx0', 'gains', 'gains_P0')}
    P, null, st = m._ptr, m._ptr(None), m._stream()

    def gains_call(key, k, p):
        return lambda: _lib.check(m.lib.mpcb_solve_gains(m._h, B, P(xbar), P(ubar), null, null, null, 0, k, p,
                                                         P(sts[key]), st))
    variants = {
        'solve_iterate': lambda: _lib.check(m.lib.mpcb_solve_iterate(
            m._h, B, P(x0), 12, P(xbar), P(ubar), P(xr), xr_sb, P(ur), 0, null, 0, P(u0), P(X), P(U),
            P(sts['solve_iterate']), st)),
        'vjp_gx0': lambda: _lib.check(m.lib.mpcb_solve_vjp(m._h, B, P(xbar), P(ubar), null, null, 0, P(gX), P(gU),
                                                           P(gx0), null, null, P(sts['vjp_gx0']), st)),
        'gains': gains_call('gains', P(K), P(P0)),
        'gains_P0': gains_call('gains_P0', null, P(P0)),     # without the N nu nx stores of K
    }
    meds, mins = _time(variants, runs, warmup, inner, repeats, rotate)
    out = dict(shape=name, B=B, N=N, dtype=dtype, runs=runs, inner=inner, repeats=repeats, order=list(meds),
               K_bytes=K.numel() * K.element_size(), **{f'{k}_status_ok': int((v == 0).sum()) for k, v in sts.items()})
    return _report(out, meds, mins, 'vjp_gx0')


def bench_full17(runs, warmup, inner, repeats, rotate=0, B=4096, N=60, dtype='f64'):
    import numpy as np
    import torch

    from mpc_blaster_amd import BatchedMPC, MPCConfig, _lib
    rng = np.random.default_rng(1017)
    x0 = np.zeros((B, 17))
    x0[:, 0:3] = rng.uniform(-1, 1, (B, 3))
    x0[:, 2] += 3.5
    x0[:, 3:6] = rng.uniform(-0.17, 0.17, (B, 3))
    x0[:, 6:9] = rng.uniform(-0.5, 0.5, (B, 3))
    x0[:, 9:12] = rng.uniform(-0.087, 0.087, (B, 3))
    xref = np.zeros((1, N + 1, 17))
    xref[..., 2], xref[..., 14] = 3.5, 0.2
    uref = np.zeros((1, N, 6))
    uref[..., :4] = 22.0725
    p = np.zeros((B, 25))
    p[:, :24] = rng.uniform(-0.5, 0.5, (B, 24))
    p[:, 24] = 2.2 * 9.81
    cfg = MPCConfig.full(N=N, dtype=dtype)
    m = BatchedMPC(cfg, max_batch=B)
    dt, dev = cfg.torch_dtype, m._tdev
    x0, xr, ur, pt = (torch.as_tensor(a, dtype=dt, device=dev) for a in (x0, xref, uref, p))
    m.set_params(pt)
    m.solve(x0, xr, ur)
    xbar, ubar = m.get_state_trajectory().clone(), m.get_input_trajectory().clone()
    gen = torch.Generator(device=dev).manual_seed(1017)
    gX = torch.randn((B, N + 1, 17), dtype=dt, device=dev, generator=gen)
    gU = torch.randn((B, N, 6), dtype=dt, device=dev, generator=gen)
    fixed = (torch.rand((B, N, 6), device=dev, generator=gen) < 0.5).to(torch.uint8)
    u0 = torch.empty((B, 6), dtype=dt, device=dev)
    X, U = torch.empty_like(xbar), torch.empty_like(ubar)
    gx0 = torch.empty((B, 17), dtype=dt, device=dev)
    K = torch.empty((B, N, 6, 17), dtype=dt, device=dev)
    P0 = torch.empty((B, 17, 17), dtype=dt, device=dev)
    sts = {k: torch.empty((B,), dtype=torch.int32, device=dev)
           for k in ('solve_iterate', 'vjp17_gx0', 'gains', 'gains_masked', 'gains_P0')}
    P, null, st = m._ptr, m._ptr(None), m._stream()

    def gains_call(key, fx, k, p_):
        return lambda: _lib.check(m.lib.mpcb_solve_gains(m._h, B, P(xbar), P(ubar), null, fx, null, 0, k, p_,
                                                         P(sts[key]), st))
    variants = {
        'solve_iterate': lambda: _lib.check(m.lib.mpcb_solve_iterate(
            m._h, B, P(x0), 17, P(xbar), P(ubar), P(xr), 0, P(ur), 0, null, 0, P(u0), P(X), P(U),
            P(sts['solve_iterate']), st)),
        'vjp17_gx0': lambda: _lib.check(m.lib.mpcb_solve_vjp17(
            m._h, B, P(xbar), P(ubar), null, null, null, null, 0, null, 0, P(gX), P(gU), P(gx0), null, null,
            null, null, null, P(sts['vjp17_gx0']), st)),
        'gains': gains_call('gains', null, P(K), P(P0)),
        'gains_masked': gains_call('gains_masked', P(fixed), P(K), P(P0)),
        'gains_P0': gains_call('gains_P0', null, null, P(P0)),
    }
    meds, mins = _time(variants, runs, warmup, inner, repeats, rotate)
    out = dict(shape='full17', B=B, N=N, dtype=dtype, runs=runs, inner=inner, repeats=repeats, order=list(meds),
               K_bytes=K.numel() * K.element_size(), **{f'{k}_status_ok': int((v == 0).sum()) for k, v in sts.items()})
    return _report(out, meds, mins, 'vjp17_gx0')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--inner', type=int, default=3, help='calls per event pair')
    ap.add_argument('--repeats', type=int, default=3, help='repetitions of the whole measurement')
    ap.add_argument('--rotate', type=int, default=0,
                    help='start the alternation at the variant of this index (the order of the variants '
                         'is part of what they are measured under)')
    ap.add_argument('--shapes', default='c2,c3')
    ap.add_argument('--full17', action='store_true',
                    help='time the 17/6 model (4096 x N = 60, fp64) instead of the 12/4 shapes')
    a = ap.parse_args()
    if a.full17:
        bench_full17(a.runs, a.warmup, a.inner, a.repeats, a.rotate)
        return
    for name in a.shapes.split(','):
        bench(name, a.runs, a.warmup, a.inner, a.repeats, a.rotate)


if __name__ == '__main__':
    main()
