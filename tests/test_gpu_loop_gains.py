"""closed_loop(resolve_every=h, feedback=...) on the GPU: a solve every h plant steps, the solve's
own inputs (or the RTI feedback law u = U_j + K_j (x - X_j) over mpcb_solve_gains) in between,
against a NumPy loop over the oracle's ``mpc_solve(mode='iterate')``, tests/gains_ref.py and the
oracle's plant step.  fp64, 12/4 with the input box; the bound is that of
tests/test_gpu_parity.py test_closed_loop_matches_oracle_fp64 (1e-8 per step on the control and on
the state, in the project's metric).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gains_ref import gains_ref, relerr   # noqa: E402
from vjp_ref import vjp_case   # noqa: E402

from oracle.model import Params   # noqa: E402
from oracle.ocp import OcpSpec, mpc_solve   # noqa: E402
from oracle.rk4 import rk4_step   # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

B, N, NSIM, H = 3, 5, 6, 3
LB, UB = np.full(4, 5.0), np.full(4, 40.0)   # (on this draw the active set converges: nothing is handed over)
ON_BOUND = 1e-9   # the oracle's U is ubar + (bound - ubar): on the bound up to rounding


def _spec():
    return OcpSpec(N=N, lbu=LB, ubu=UB)


def _case():
    return vjp_case(B, N, _spec())


def reference_loop(c, feedback):
    """(X_sim [B,NSIM+1,12], U_sim [B,NSIM,4], clamped components of the solves, clipped controls)."""
    spec = _spec()
    xbar, ubar, x = c['xbar'].copy(), c['ubar'].copy(), c['x0'].copy()
    Xs, Us = [x], []
    nfix = nclip = 0
    for i in range(NSIM):
        j = i % H
        if j == 0:
            o = mpc_solve(x, c['xref'], c['uref'], spec, mode='iterate', xbar=xbar, ubar=ubar)
            assert (o['status'] == 0).all() and not o['fallback'].any()
            fixed = (o['U'] <= LB + ON_BOUND) | (o['U'] >= UB - ON_BOUND)
            nfix += int(fixed.sum())
            if feedback:
                K = gains_ref(xbar, ubar, fixed, spec)['K']
            xbar, ubar = o['X'], o['U']
        u = ubar[:, j]
        if feedback:
            u = u + np.einsum('bmi,bi->bm', K[:, j], x - xbar[:, j])
        nclip += int(((u < LB) | (u > UB)).sum())
        u = np.clip(u, LB, UB)
        x = rk4_step(x, u, spec.dt, Params())
        Us.append(u)
        Xs.append(x)
    return np.stack(Xs, axis=1), np.stack(Us, axis=1), nfix, nclip


@pytest.mark.parametrize('feedback', [False, True])
def test_held_loop_matches_oracle_fp64(feedback):
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    from mpc_blaster_amd.closed_loop import closed_loop
    c = _case()
    Xr, Ur, nfix, nclip = reference_loop(c, feedback)
    m = BatchedMPC(MPCConfig(N=N, lbu=LB, ubu=UB), max_batch=B)
    Xs, Us, st = closed_loop(m, c['x0'], c['xref'], c['uref'], NSIM, xbar=c['xbar'], ubar=c['ubar'],
                             resolve_every=H, feedback=feedback)
    torch.cuda.synchronize()
    Xs, Us = Xs.cpu().numpy(), Us.cpu().numpy()
    assert (st.cpu().numpy() == 0).all()
    eu = max(relerr(Us[:, i], Ur[:, i]).max() for i in range(NSIM))
    ex = max(relerr(Xs[:, i + 1], Xr[:, i + 1]).max() for i in range(NSIM))
    print(f'held loop feedback={feedback}: u {eu:.2e}  x {ex:.2e} (bound 1e-8); {nfix} clamped components in the '
          f'solves, {nclip} controls clipped')
    assert nfix > 0
    assert eu < 1e-8 and ex < 1e-8
    assert (Us >= LB).all() and (Us <= UB).all()
    if feedback:   # the feedback term is not nothing
        Uh = reference_loop(c, False)[1]
        assert np.abs(Ur - Uh).max() > 1e-4


def test_defaults_are_the_loop_as_it_was():
    """resolve_every=1, feedback=False: the bits of a call without the new arguments."""
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    from mpc_blaster_amd.closed_loop import closed_loop
    c = _case()
    m = BatchedMPC(MPCConfig(N=N, lbu=LB, ubu=UB), max_batch=B)
    a = closed_loop(m, c['x0'], c['xref'], c['uref'], NSIM, xbar=c['xbar'], ubar=c['ubar'])
    b = closed_loop(m, c['x0'], c['xref'], c['uref'], NSIM, xbar=c['xbar'], ubar=c['ubar'], resolve_every=1,
                    feedback=False)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    with pytest.raises(ValueError):
        closed_loop(m, c['x0'], c['xref'], c['uref'], NSIM, resolve_every=N + 1)
    with pytest.raises(ValueError):
        closed_loop(m, c['x0'], c['xref'], c['uref'], NSIM, resolve_every=0)
    # an f32 17/6 input-box handle has no default tolerance: refused before the loop starts
    import vjp17_ref as vr
    mf = BatchedMPC(MPCConfig.full(N=N, dtype='f32', lbu=vr.LBU17, ubu=vr.UBU17), max_batch=B)
    with pytest.raises(ValueError, match='active_tol'):
        closed_loop(mf, np.zeros((B, 17)), np.zeros((1, N + 1, 17)), np.zeros((1, N, 6)), NSIM, resolve_every=H,
                    feedback=True)


def test_held_loop_with_a_tolerance_is_the_loop_that_reads_U():
    """active_tol is forwarded: on this draw the mask by 1e-9 is the set the library reads from U."""
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    from mpc_blaster_amd.closed_loop import closed_loop
    c = _case()
    m = BatchedMPC(MPCConfig(N=N, lbu=LB, ubu=UB), max_batch=B)
    kw = dict(xbar=c['xbar'], ubar=c['ubar'], resolve_every=H, feedback=True)
    a = closed_loop(m, c['x0'], c['xref'], c['uref'], NSIM, **kw)
    b = closed_loop(m, c['x0'], c['xref'], c['uref'], NSIM, active_tol=1e-9, **kw)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
