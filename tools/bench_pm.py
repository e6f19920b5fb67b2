#!/usr/bin/env python
"""Device time of mpcb_solve_iterate_pm (the RTI step with a vehicle per instance) next to
mpcb_solve_iterate_pw and mpcb_solve_iterate at the same shape, of mpcb_solve_gains_pm next to
mpcb_solve_gains, and of mpcb_sim_step_pm next to mpcb_sim_step.

``pm`` is the per-instance-model kernel with the handle's weights (the three weight pointers NULL),
``pw_null`` the kernel of mpcb_solve_iterate_pw called the same way: their ratio is what the record
(14 loads per instance, the fp64 adjugate, the model in LDS in fp64 and in registers in fp32) costs.  ``pm_w`` and ``pw`` are the
same pair with per-instance weights.  mpcb_solve_iterate is the handle's tuned path.

Shape: 4096 x N = 20, hover, in fp64 and fp32; with ``--box`` the input box [0, 65] in fp64 only
(fp32 with the box is refused by both entry points).  The iterate is one rollout-mode RTI step; the
vehicles are the handle's under mass x U(0.8, 1.25), arms and yaw coefficient x U(0.9, 1.1),
T_blast U(0, 5) and a diagonal congruence of J (e = exp(0.2 N(0, 1))), drawn on the device; the
weights as in tools/bench_pw.py.  HIP events around ``--inner`` back-to-back calls, median of
``--runs`` after ``--warmup`` calls of every variant, the variants alternating so drift hits them
alike.  Prints one JSON line per dtype.

    python tools/bench_pm.py [--box] [--batch B] [--runs 20] [--warmup 5] [--inner 5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench(dtype, box, B, runs, warmup, inner):
    import numpy as np
    import torch

    from mpc_blaster_amd import BatchedMPC, MPCConfig, _lib
    N, seed = 20, 1004 if box else 1002
    m = BatchedMPC(MPCConfig(N=N, dtype=dtype, lbu=np.zeros(4) if box else None,
                             ubu=np.full(4, 65.0) if box else None), max_batch=B)
    inp = m.gen_inputs(B, seed=seed, ref='hover', wind=False)
    m.solve(inp['x0'], inp['xref'], inp['uref'])
    xbar, ubar = m.get_state_trajectory().clone(), m.get_input_trajectory().clone()
    x0, xr, ur = inp['x0'], inp['xref'], inp['uref']
    dev, dt = xbar.device, xbar.dtype
    gen = torch.Generator(device=dev).manual_seed(seed)

    def uni(lo, hi):
        return lo + (hi - lo) * torch.rand((B,), dtype=dt, device=dev, generator=gen)

    def congruent(W, sigma):
        W = torch.as_tensor(np.asarray(W, dtype=np.float64), dtype=dt, device=dev)
        e = torch.exp(sigma * torch.randn((B, W.shape[0]), dtype=dt, device=dev, generator=gen))
        return (W[None] * e[:, :, None] * e[:, None, :]).contiguous()
    Qw, Rw, QNw = congruent(m.cfg.Q, 0.35), congruent(m.cfg.R, 0.35), congruent(m.cfg.QN, 0.35)
    model = m.pack_model(B, mass=m.cfg.mass * uni(0.8, 1.25), lx=m.cfg.lx * uni(0.9, 1.1), ly=m.cfg.ly * uni(0.9, 1.1),
                         c=m.cfg.c * uni(0.9, 1.1), t_blast=uni(0.0, 5.0), J=congruent(m.cfg.J, 0.2))

    def outs():
        return (torch.empty((B, 4), dtype=dt, device=dev), torch.empty_like(xbar), torch.empty_like(ubar),
                torch.empty((B,), dtype=torch.int32, device=dev))
    o = {k: outs() for k in ('solve_iterate', 'pw', 'pw_null', 'pm', 'pm_w')}
    xo, xo_pm = torch.empty_like(x0), torch.empty_like(x0)
    K, P0 = torch.empty((B, N, 4, 12), dtype=dt, device=dev), torch.empty((B, 12, 12), dtype=dt, device=dev)
    gst = {k: torch.empty((B,), dtype=torch.int32, device=dev) for k in ('gains', 'gains_pm')}
    P, null, st = m._ptr, m._ptr(None), m._stream()
    u_sim = ubar[:, 0].contiguous()

    def pm_call(k, W, md):
        W = [(P(w), n) if w is not None else (null, 0) for w, n in zip(W, (144, 16, 144))]
        head = [m._h, B, P(x0), 12, P(xbar), P(ubar), P(xr), 0, P(ur), 0, null, 0, W[0][0], W[0][1], W[1][0], W[1][1],
                W[2][0], W[2][1]]
        tail = [P(v) for v in o[k]] + [st]
        if md is None:
            return lambda: _lib.check(m.lib.mpcb_solve_iterate_pw(*head, *tail))
        return lambda: _lib.check(m.lib.mpcb_solve_iterate_pm(*head, P(md), 14, *tail))
    Ug = P(o['pm'][2]) if box else null   # the gains' active set: the per-instance-model solve's U
    variants = {
        'solve_iterate': lambda: _lib.check(m.lib.mpcb_solve_iterate(
            m._h, B, P(x0), 12, P(xbar), P(ubar), P(xr), 0, P(ur), 0, null, 0, *[P(v) for v in o['solve_iterate']],
            st)),
        'pw': pm_call('pw', (Qw, Rw, QNw), None),
        'pw_null': pm_call('pw_null', (None, None, None), None),
        'pm': pm_call('pm', (None, None, None), model),
        'pm_w': pm_call('pm_w', (Qw, Rw, QNw), model),
        'gains': lambda: _lib.check(m.lib.mpcb_solve_gains(m._h, B, P(xbar), P(ubar), Ug, null, null, 0, P(K), P(P0),
                                                           P(gst['gains']), st)),
        'gains_pm': lambda: _lib.check(m.lib.mpcb_solve_gains_pm(m._h, B, P(xbar), P(ubar), Ug, null, null, 0,
                                                                 P(model), 14, P(K), P(P0), P(gst['gains_pm']), st)),
        'sim_step': lambda: _lib.check(m.lib.mpcb_sim_step(m._h, B, P(x0), P(u_sim), null, 0, float(m.cfg.dt), P(xo),
                                                           st)),
        'sim_step_pm': lambda: _lib.check(m.lib.mpcb_sim_step_pm(m._h, B, P(x0), P(u_sim), null, 0, P(model), 14,
                                                                 float(m.cfg.dt), P(xo_pm), st)),
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
    U = o['pm'][2]
    out = dict(shape='c2-box' if box else 'c2', B=B, N=N, dtype=dtype, box=box, runs=runs, inner=inner,
               **{f'{k}_ms': round(v, 4) for k, v in med.items()},
               **{f'{k}_min_ms': round(min(v), 4) for k, v in t.items()},
               pm_over_pw_null=round(med['pm'] / med['pw_null'], 3),
               pm_w_over_pw=round(med['pm_w'] / med['pw'], 3),
               pm_over_solve=round(med['pm'] / med['solve_iterate'], 3),
               gains_pm_over_gains=round(med['gains_pm'] / med['gains'], 3),
               sim_step_pm_over_sim_step=round(med['sim_step_pm'] / med['sim_step'], 3),
               **{f'{k}_status_ok': int((v[3] == 0).sum()) for k, v in o.items()},
               **{f'{k}_status_ok': int((v == 0).sum()) for k, v in gst.items()},
               sim_step_pm_finite=bool(torch.isfinite(xo_pm).all()),
               clamped_fraction=(float(((U <= 0.0) | (U >= 65.0)).double().mean()) if box else 0.0))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--box', action='store_true', help='the input box [0, 65] (fp64 only)')
    ap.add_argument('--batch', type=int, default=4096, help='instances')
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--inner', type=int, default=5, help='launches per event pair')
    a = ap.parse_args()
    for dtype in (('f64',) if a.box else ('f64', 'f32')):
        bench(dtype, a.box, a.batch, a.runs, a.warmup, a.inner)


if __name__ == '__main__':
    main()
