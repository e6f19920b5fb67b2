#!/usr/bin/env python
"""The penalty of the state rows of mpcb_solve_vjp17_sx (mpcb_full.h SX17_RHO), measured on the device.

For rho in 1e6, 1e8 (the library's), 1e10: the device's statuses and its error against the dense KKT
reference (tests/vjp17x_ref.py ``dense_x``; the project's metric, worst instance and output) on the
cases of the tests: synthetic masks at (B, N) = (5, 3) and (7, 17), and the oracle's masks on the
state-box draws at (6, 8), (5, 12) and (8, 20).  The device does not report its pass counts; the
NumPy model of the recursion at the same rho does (``al_x``), and its statuses stand next to the
device's.  DESIGN.md records the table.

The other penalties need libraries of their own: ``--build`` compiles them with -DMPCB_SX17_RHO into
mpc_blaster_amd/variants/ (not tracked); each rho then runs in a process of its own under MPCB_LIB.

    python tools/sx_rho_sweep.py --build      # on the build machine
    python tools/sx_rho_sweep.py              # on the GPU
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
RHOS = ('1e6', '1e8', '1e10')


def _lib(rho):
    return None if rho == '1e8' else os.path.join(ROOT, 'mpc_blaster_amd', 'variants', f'libmpcblaster_sxrho{rho}.so')


def one(rho):
    import numpy as np
    import torch
    import vjp17_ref as vr
    import vjp17x_ref as xr
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    from oracle.full import FullSpec
    cases = [('synthetic', B, N) for B, N in ((5, 3), (7, 17))] + [('end to end', B, N) for B, N in ((6, 8), (5, 12), (8, 20))]
    for kind, B, N in cases:
        if kind == 'synthetic':
            c, fixed, fixed_x = xr.synth_case(B, N)
            spec = FullSpec(N=N)
        else:
            spec, c = xr.sbox_case(B, N)
            fixed, fixed_x = c['fixed'], c['fixed_x']
        args = (c['xbar'], c['ubar'], c['p'], fixed, fixed_x, c['gX'], c['gU'], spec)
        dense, al = xr.dense_x(*args), xr.al_x(*args, rho=float(rho))
        m = BatchedMPC(MPCConfig.full(N=N), max_batch=B)
        m.set_params(c['p'])
        out = m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], fixed=fixed, fixed_x=fixed_x)
        torch.cuda.synchronize()
        got = {k: out[k].cpu().numpy() for k in xr.KEYS + ('status',)}
        err = np.max([vr.relerr(got[k], dense[k]) for k in xr.KEYS], axis=0)
        conv = got['status'] == 0
        print(json.dumps(dict(rho=rho, case=kind, B=B, N=N, device_status=got['status'].tolist(),
                              model_status=al['status'].tolist(), model_passes=al['passes'].tolist(),
                              worst_error_converged=float(err[conv].max()) if conv.any() else None,
                              error_per_instance=[float(f'{e:.3g}') for e in err])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--build', action='store_true')
    ap.add_argument('--one', default=None, help='(internal) run one penalty in this process')
    a = ap.parse_args()
    if a.build:
        from mpc_blaster_amd.build import build
        for rho in RHOS:
            if _lib(rho):
                os.makedirs(os.path.dirname(_lib(rho)), exist_ok=True)
                build(force=True, verbose=False, out=_lib(rho), extra=[f'-DMPCB_SX17_RHO={rho}'])
        return
    if a.one:
        one(a.one)
        return
    for rho in RHOS:
        env = dict(os.environ)
        if _lib(rho):
            env['MPCB_LIB'] = _lib(rho)
        subprocess.run([sys.executable, os.path.abspath(__file__), '--one', rho], env=env, check=True, timeout=300)


if __name__ == '__main__':
    main()
