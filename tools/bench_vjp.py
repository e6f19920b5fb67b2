#!/usr/bin/env python
"""Device time of mpcb_solve_vjp next to mpcb_solve_iterate at the same shape.

The backward pass of the torch layer (mpc_blaster_amd/autograd.py) is one mpcb_solve_vjp call, the
forward pass one mpcb_solve_iterate call, so their ratio is what a gradient costs on top of a
solve.  The product runs the pass structure of the single-kernel solver (mpcb_solve.hip: nominal,
backward Riccati, forward, one launch), so that path (a handle created under
MPCB_SPLIT_MIN_BATCH above the batch; MPCB_BOX_IMPL=v1 with the box) is timed as well, next to the
default path of the handle.  Shapes: c2 (4096 x N = 20, fp64), c3 (65536 x N = 20, fp32, sine
references) and one 65536-instance shard of c4 (N = 30, fp32, input box [0, 65]).

The iterate is one rollout-mode RTI step; U of the timed solve_iterate gives the product's active
set; the cotangents are standard normal.  HIP events around ``--inner`` back-to-back calls, median
of ``--runs`` after ``--warmup`` calls of every variant, the variants alternating so drift hits
them alike.  Prints one JSON line per shape.

``--weights`` adds mpcb_solve_vjp_w with all six outputs (X and U: the timed solve's) and its ratio
to the plain product on the same build.

``--full17`` times mpcb_solve_vjp17 instead (the 17/6 model at 4096 x N = 60, fp64, the shape of
tools/bench_full17.py), with an empty and a half-full mask and, with ``--weights``, all six
outputs, next to the unboxed mpcb_solve_iterate of the same handle.

``--full17 --state-rows`` times mpcb_solve_vjp17_sx on the 17/6 state-box bench draws (the draws of
tools/bench_full17.py --bounds all, 4096 x N = 60, fp64) with the two masks of a real solve_iterate
step, next to the same call without state rows (fixed_x = NULL: the kernels of mpcb_solve_vjp17)
and the state-box solve itself.  The device does not report its pass counts, so they come from the
NumPy model of the recursion (tests/vjp17x_ref.py ``al_x``) on the first ``--model`` instances,
whose statuses are compared with the device's.

    python tools/bench_vjp.py [--runs 20] [--warmup 5] [--inner 5] [--shapes c2,c3,c4] [--weights] [--full17]
                              [--state-rows [--model 64]]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    # name: (B, N, dtype, references, box, seed)
    'c2': (4096, 20, 'f64', 'hover', False, 1002),
    'c3': (65536, 20, 'f32', 'sine', False, 1003),
    'c4': (65536, 30, 'f32', 'hover', True, 1004),
}


def _handle(N, dtype, box, B, env):
    import numpy as np

    from mpc_blaster_amd import BatchedMPC, MPCConfig
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return BatchedMPC(MPCConfig(N=N, dtype=dtype, lbu=np.zeros(4) if box else None,
                                    ubu=np.full(4, 65.0) if box else None), max_batch=B)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def bench(name, runs, warmup, inner, weights=False):
    import torch

    from mpc_blaster_amd import _lib
    B, N, dtype, ref, box, seed = SHAPES[name]
    m = _handle(N, dtype, box, B, {})
    single_env = {'MPCB_BOX_IMPL': 'v1'} if box else {'MPCB_SPLIT_MIN_BATCH': str(1 << 40)}
    ms1 = _handle(N, dtype, box, B, single_env)
    assert ms1.path == 'fused' and (box or m.path == 'split')
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
    gx0, gxr, gur = torch.empty((B, 12), dtype=dt, device=dev), torch.empty_like(xbar), torch.empty_like(ubar)
    st_s = torch.empty((B,), dtype=torch.int32, device=dev)
    st_v = torch.empty((B,), dtype=torch.int32, device=dev)
    P, null, st = m._ptr, m._ptr(None), m._stream()

    # (the single-kernel solver gets outputs of its own: the product reads the default path's U)
    o1 = (torch.empty_like(u0), torch.empty_like(X), torch.empty_like(U), torch.empty_like(st_s))

    def solve_call(hd, o):
        return lambda: _lib.check(hd.lib.mpcb_solve_iterate(hd._h, B, P(x0), 12, P(xbar), P(ubar), P(xr), xr_sb,
                                                            P(ur), 0, null, 0, P(o[0]), P(o[1]), P(o[2]), P(o[3]), st))
    variants = {
        'solve_iterate': solve_call(m, (u0, X, U, st_s)),
        'solve_iterate_single': solve_call(ms1, o1),
        'vjp': lambda: _lib.check(m.lib.mpcb_solve_vjp(m._h, B, P(xbar), P(ubar), P(U) if box else null, null, 0,
                                                       P(gX), P(gU), P(gx0), P(gxr), P(gur), P(st_v), st)),
    }
    if weights:   # all six gradients in one launch; X and U are the timed solve's outputs
        gQ, gR = torch.empty((B, 12, 12), dtype=dt, device=dev), torch.empty((B, 4, 4), dtype=dt, device=dev)
        gQN, st_w = torch.empty_like(gQ), torch.empty_like(st_v)
        variants['vjp_w'] = lambda: _lib.check(m.lib.mpcb_solve_vjp_w(
            m._h, B, P(xbar), P(ubar), P(X), P(U), P(xr), xr_sb, P(ur), 0, null, 0, P(gX), P(gU), P(gx0), P(gxr),
            P(gur), P(gQ), P(gR), P(gQN), P(st_w), st))
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
    out = dict(shape=name, B=B, N=N, dtype=dtype, box=box, runs=runs, inner=inner,
               **{f'{k}_ms': round(v, 4) for k, v in med.items()},
               **{f'{k}_min_ms': round(min(v), 4) for k, v in t.items()},
               vjp_over_solve=round(med['vjp'] / med['solve_iterate'], 3),
               vjp_over_single=round(med['vjp'] / med['solve_iterate_single'], 3),
               solve_status_ok=int((st_s == 0).sum()), vjp_status_ok=int((st_v == 0).sum()),
               clamped_fraction=(float(((U <= 0.0) | (U >= 65.0)).double().mean()) if box else 0.0))
    if weights:
        out.update(vjp_w_over_vjp=round(med['vjp_w'] / med['vjp'], 3), vjp_w_status_ok=int((st_w == 0).sum()))
    print(json.dumps(out), flush=True)
    return out


def bench_full17(runs, warmup, inner, weights=False, B=4096, N=60, dtype='f64'):
    """mpcb_solve_vjp17 next to the unboxed mpcb_solve_iterate of the same handle: 4096 x N = 60,
    fp64, the draws of tools/bench_full17.py (random x0 around hover, per-instance POC parameters).
    A synthetic mask (about half of the components clamped) is timed as well: it costs what the
    empty one costs, the mask being an operand of selects."""
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
    gx0, gxr, gur = torch.empty((B, 17), dtype=dt, device=dev), torch.empty_like(xbar), torch.empty_like(ubar)
    gQ, gR = torch.empty((B, 17, 17), dtype=dt, device=dev), torch.empty((B, 6, 6), dtype=dt, device=dev)
    gQN = torch.empty_like(gQ)
    sts = {k: torch.empty((B,), dtype=torch.int32, device=dev) for k in ('solve_iterate', 'vjp17', 'vjp17_masked', 'vjp17_w')}
    P, null, st = m._ptr, m._ptr(None), m._stream()

    def vjp_call(key, fx, wg):
        w = (P(gQ), P(gR), P(gQN)) if wg else (null, null, null)
        return lambda: _lib.check(m.lib.mpcb_solve_vjp17(
            m._h, B, P(xbar), P(ubar), fx, P(X) if wg else null, P(U) if wg else null, P(xr) if wg else null, 0,
            P(ur) if wg else null, 0, P(gX), P(gU), P(gx0), P(gxr), P(gur), *w, P(sts[key]), st))
    variants = {
        'solve_iterate': lambda: _lib.check(m.lib.mpcb_solve_iterate(
            m._h, B, P(x0), 17, P(xbar), P(ubar), P(xr), 0, P(ur), 0, null, 0, P(u0), P(X), P(U),
            P(sts['solve_iterate']), st)),
        'vjp17': vjp_call('vjp17', null, False),
        'vjp17_masked': vjp_call('vjp17_masked', P(fixed), False),
    }
    if weights:
        variants['vjp17_w'] = vjp_call('vjp17_w', null, True)
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
    out = dict(shape='full17', B=B, N=N, dtype=dtype, box=False, runs=runs, inner=inner,
               **{f'{k}_ms': round(v, 4) for k, v in med.items()},
               **{f'{k}_min_ms': round(min(v), 4) for k, v in t.items()},
               vjp17_over_solve=round(med['vjp17'] / med['solve_iterate'], 3),
               vjp17_masked_over_solve=round(med['vjp17_masked'] / med['solve_iterate'], 3),
               **{f'{k}_status_ok': int((sts[k] == 0).sum()) for k in variants})
    if weights:
        out.update(vjp17_w_over_solve=round(med['vjp17_w'] / med['solve_iterate'], 3),
                   vjp17_w_over_vjp17=round(med['vjp17_w'] / med['vjp17'], 3))
    print(json.dumps(out), flush=True)
    return out


def bench_full17_sx(runs, warmup, inner, model=64, B=4096, N=60):
    """mpcb_solve_vjp17_sx with the masks of a real state-box solve (module docstring)."""
    import numpy as np
    import torch

    from mpc_blaster_amd import BatchedMPC, MPCConfig, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, 'tools'), os.path.join(root, 'tests')]
    from sbox_stall_study import draws   # the 17/6 bench draws (tools/bench_full17.py --bounds all)
    x0, xref, uref, p, lbu, ubu, lbx, ubx = draws(N, B)
    m = BatchedMPC(MPCConfig.full(N=N, lbu=lbu, ubu=ubu, lbx=lbx, ubx=ubx), max_batch=B)
    dt, dev = m.dtype, m._tdev
    x0d, xr, ur, pt = (torch.as_tensor(a, dtype=dt, device=dev) for a in (x0, xref, uref, p))
    m.set_params(pt)
    m.solve(x0d, xr, ur)   # the iterate: one rollout-mode step
    xbar, ubar = m.get_state_trajectory().clone(), m.get_input_trajectory().clone()
    m.solve_iterate(x0d, xbar, ubar, xr, ur)
    X, U, sst = m.get_state_trajectory().clone(), m.get_input_trajectory().clone(), m.get_status().clone()
    fixed, fixed_x = m.active_mask17(U), m.active_mask17x(X)
    gen = torch.Generator(device=dev).manual_seed(1017)
    gX = torch.randn((B, N + 1, 17), dtype=dt, device=dev, generator=gen)
    gU = torch.randn((B, N, 6), dtype=dt, device=dev, generator=gen)
    u0o, Xo, Uo = torch.empty((B, 6), dtype=dt, device=dev), torch.empty_like(X), torch.empty_like(U)
    gx0, gxr, gur = torch.empty((B, 17), dtype=dt, device=dev), torch.empty_like(xbar), torch.empty_like(ubar)
    sts = {k: torch.empty((B,), dtype=torch.int32, device=dev) for k in ('solve_iterate', 'vjp17', 'vjp17_sx')}
    P, null, st = m._ptr, m._ptr(None), m._stream()

    def sx_call(key, fxx):
        return lambda: _lib.check(m.lib.mpcb_solve_vjp17_sx(
            m._h, B, P(xbar), P(ubar), P(fixed), fxx, null, null, null, 0, null, 0, null, 0, null, 0, null, 0,
            P(gX), P(gU), P(gx0), P(gxr), P(gur), null, null, null, P(sts[key]), st))
    variants = {
        'solve_iterate': lambda: _lib.check(m.lib.mpcb_solve_iterate(
            m._h, B, P(x0d), 17, P(xbar), P(ubar), P(xr), 0, P(ur), 0, null, 0, P(u0o), P(Xo), P(Uo),
            P(sts['solve_iterate']), st)),
        'vjp17': sx_call('vjp17', null),
        'vjp17_sx': sx_call('vjp17_sx', P(fixed_x)),
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
    solved = (sst == 0).cpu().numpy()
    rows = fixed_x.sum(dim=(1, 2)).cpu().numpy()
    dst = sts['vjp17_sx'].cpu().numpy()
    out = dict(shape='full17_state_rows', B=B, N=N, dtype='f64', runs=runs, inner=inner,
               **{f'{k}_ms': round(v, 4) for k, v in med.items()},
               **{f'{k}_min_ms': round(min(v), 4) for k, v in t.items()},
               sx_over_vjp17=round(med['vjp17_sx'] / med['vjp17'], 3),
               sx_over_solve=round(med['vjp17_sx'] / med['solve_iterate'], 3),
               solve_status_ok=int(solved.sum()),
               rows_per_instance=[int(rows[solved].min()), float(np.median(rows[solved])), int(rows[solved].max())],
               sx_status_counts_of_solved={str(k): int(((dst == k) & solved).sum()) for k in np.unique(dst[solved])})
    if model > 0:   # the pass counts of the recursion's NumPy model on the first instances
        import vjp17x_ref as xr
        from oracle.full import FullSpec
        n = min(model, B)
        f = lambda a: a[:n].cpu().numpy()   # noqa: E731
        al = xr.al_x(f(xbar), f(ubar), p[:n], f(fixed), f(fixed_x), f(gX), f(gU),
                     FullSpec(N=N, lbu=lbu, ubu=ubu, lbx=lbx, ubx=ubx))
        ok = solved[:n]
        out.update(model_instances=int(ok.sum()),
                   model_passes_hist=np.bincount(al['passes'][ok], minlength=xr.SX17_ITERS + 1).tolist(),
                   model_status_equal=int((al['status'][ok] == dst[:n][ok]).sum()))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--inner', type=int, default=5, help='launches per event pair')
    ap.add_argument('--shapes', default='c2,c3,c4')
    ap.add_argument('--weights', action='store_true',
                    help='also time mpcb_solve_vjp_w (the weight gradients gQ, gR, gQN in the same launch)')
    ap.add_argument('--full17', action='store_true',
                    help='time mpcb_solve_vjp17 (17/6 model, 4096 x N = 60, fp64) instead of the 12/4 shapes')
    ap.add_argument('--state-rows', action='store_true',
                    help='with --full17: time mpcb_solve_vjp17_sx on the state-box bench draws')
    ap.add_argument('--model', type=int, default=64,
                    help='with --state-rows: instances whose pass counts the NumPy model reports (0: none)')
    a = ap.parse_args()
    if a.state_rows:
        if not a.full17:
            ap.error('--state-rows belongs to --full17')
        bench_full17_sx(a.runs, a.warmup, a.inner, a.model)
        return
    if a.full17:
        bench_full17(a.runs, a.warmup, a.inner, a.weights)
        return
    for name in a.shapes.split(','):
        bench(name, a.runs, a.warmup, a.inner, a.weights)


if __name__ == '__main__':
    main()
