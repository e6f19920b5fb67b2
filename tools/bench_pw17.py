#!/usr/bin/env python3
"""The per-instance-weight 17/6 calls next to their shared-weight twins, on one handle and one set
of inputs: tools/bench_full17.py's problem (the reference OCP, B = 4096, N = 60) in iterate mode,
the iterate being the (X, U) of one rollout solve.

    python tools/bench_pw17.py [--bounds none|input] [--dtype f64|f32] [--batch 4096] [--N 60]
                               [--rounds 7] [--reps 5]

Timed, alternating within every round so that drift of the shared machine hits all alike, each
window between two device events around ``reps`` calls:
  solve    mpcb_solve_iterate                       (the shared-weight kernels)
  pw       mpcb_solve_iterate_pw17, Q, R, QN [B, ...] per instance (a congruence of the handle's)
  pw_bc    mpcb_solve_iterate_pw17, the handle's own matrices broadcast (stride 0): the same QP as
           ``solve``, bit for bit, through the PW kernel
  vjp      mpcb_solve_vjp17 with the weight outputs          (random mask, about half clamped)
  vjp_pw   mpcb_solve_vjp_pw17, per-instance weights, the same outputs
Prints one JSON line: the median ms per call of each, min and max over the rounds, and the ratios
pw / solve, pw_bc / solve, vjp_pw / vjp.  With per-instance weights the interior point solves B
other QPs, so with a box ``pw`` also carries their iteration counts; ``pw_bc`` is the like-for-like
cost of the PW kernel.  Compulsory extra traffic: 614 weights per instance against about
23 x 17 x N linearisation values per pass.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--N', type=int, default=60)
    ap.add_argument('--dtype', default='f64', choices=['f64', 'f32'])
    ap.add_argument('--bounds', default='none', choices=['none', 'input'])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sigma', type=float, default=0.3, help='spread of the per-instance congruence')
    args = ap.parse_args()
    import torch
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    assert torch.cuda.is_available(), 'bench_pw17 needs the GPU'
    B, N = args.batch, args.N
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
    kw = {}
    if args.bounds == 'input':
        kw.update(lbu=np.array([0.0, 0.0, 0.0, 0.0, -0.0872665, -0.0872665]),
                  ubu=np.array([65.0, 65.0, 65.0, 65.0, 0.0872665, 0.0872665]))
    cfg = MPCConfig.full(N=N, dtype=args.dtype, **kw)
    m = BatchedMPC(cfg, max_batch=B)
    dt, dev = cfg.torch_dtype, 'cuda:0'
    T = lambda a: torch.as_tensor(a, dtype=dt, device=dev)   # noqa: E731
    x0t, xrt, urt = T(x0), T(xref), T(uref)
    m.set_params(T(p))
    # the iterate: one rollout solve's trajectories
    m.solve(x0t, xrt, urt)
    xb, ub = m.get_state_trajectory().clone(), m.get_input_trajectory().clone()
    # weights: the handle's, broadcast [1, n, n]; and a congruence of them per instance
    from oracle.full import default_Q17, default_R6
    Q0, R0 = np.asarray(default_Q17(), dtype=np.float64), np.asarray(default_R6(), dtype=np.float64)
    Q0 = np.diag(Q0) if Q0.ndim == 1 else Q0
    R0 = np.diag(R0) if R0.ndim == 1 else R0

    def congr(W0):
        e = np.exp(0.5 * args.sigma * rng.standard_normal((B, W0.shape[0])))
        return W0[None] * e[:, :, None] * e[:, None, :]

    Wb = dict(Q=T(Q0[None]), R=T(R0[None]), QN=T(10.0 * Q0[None]))
    Wp = dict(Q=T(congr(Q0)), R=T(congr(R0)), QN=T(congr(10.0 * Q0)))
    outs = (torch.empty((B, 6), dtype=dt, device=dev), torch.empty((B, N + 1, 17), dtype=dt, device=dev),
            torch.empty((B, N, 6), dtype=dt, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
    fixed = (torch.rand((B, N, 6), device=dev, generator=torch.Generator(dev).manual_seed(5)) < 0.5).to(torch.uint8)
    gX, gU = torch.randn((B, N + 1, 17), dtype=dt, device=dev), torch.randn((B, N, 6), dtype=dt, device=dev)
    vk = dict(gX=gX, gU=gU, fixed=fixed, weights=True)

    calls = {
        'solve': lambda: m.solve_iterate(x0t, xb, ub, xrt, urt, out=outs),
        'pw': lambda: m.solve_iterate_pw17(x0t, xb, ub, xrt, urt, out=outs, **Wp),
        'pw_bc': lambda: m.solve_iterate_pw17(x0t, xb, ub, xrt, urt, out=outs, **Wb),
    }
    status = {}
    for k, f in calls.items():   # warm-up, and what each computes
        f()
        torch.cuda.synchronize()
        status[k] = np.bincount(outs[3].cpu().numpy(), minlength=5).tolist()
        if k == 'solve':
            ref_bits = [o.clone() for o in outs[:3]]
        if k == 'pw_bc':
            same = all(torch.equal(a, b) for a, b in zip(ref_bits, outs[:3]))
    Xs, Us = outs[1].clone(), outs[2].clone()
    calls['vjp'] = lambda: m.solve_iterate_vjp(xb, ub, U=Us, X=Xs, x_ref=xrt, u_ref=urt, **vk)
    calls['vjp_pw'] = lambda: m.solve_iterate_vjp_pw17(xb, ub, U=Us, X=Xs, x_ref=xrt, u_ref=urt, **vk, **Wp)
    for k in ('vjp', 'vjp_pw'):
        for _ in range(2):
            calls[k]()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.reps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({
        'metric': f'ms per call, 17/6 per-instance weights next to the shared-weight calls (B={B}, N={N})',
        'dtype': args.dtype, 'bounds': args.bounds, 'batch': B, 'N': N, 'rounds': args.rounds, 'reps': args.reps,
        'ms': {k: dict(median=med[k], min=min(v), max=max(v)) for k, v in ms.items()},
        'ratio': {'pw/solve': med['pw'] / med['solve'], 'pw_bc/solve': med['pw_bc'] / med['solve'],
                  'vjp_pw/vjp': med['vjp_pw'] / med['vjp']},
        'pw_bc_bits_equal_solve': bool(same), 'status_counts': status, 'sigma': args.sigma}))


if __name__ == '__main__':
    main()
