"""NumPy references of mpcb_solve_vjp17_sx (include/mpcb.h), the 17/6 product with active state
rows, and the draws its tests share; a helper, not a test.

The problem is the adjoint LQ problem of tests/vjp_ref.py (module docstring) over the 17/6
linearisation with one more family of constraints, dx_k[i] = 0 on every active state row (k, i),
1 <= k <= N-1.  With mu_k[i] their multipliers (zero elsewhere) the outputs are gxref_k = s Q dx_k
(QN dx_N at the end), guref_k = s R du_k and gx0 = nu_0 from nu_N = gX_N - QN dx_N,
nu_k = gX_k - s Q dx_k - mu_k + A_k' nu_{k+1}; the weight formulas are those of
tests/vjp17_ref.py on this (dx, du).

Two solvers:
 * ``dense_x``: the problem condensed onto the inputs (dx = S du, tests/vjp_ref.py ``_dense``), the
   clamped inputs masked out as there, the state rows as constraint rows C du = 0 of a KKT system
   solved with ``lstsq`` (dependent rows get the least-norm multipliers).  No recursion, no
   penalty: it shares nothing with the device's algebra.  It loses digits with the horizon as
   ``_dense`` does.
 * ``al_x``: the model of the device's recursion with the constants of mpcb_full.h (SX17_*):
   augmented-Lagrangian passes over ``oracle.ocp.riccati_solve`` with Qd = rho mask,
   qd = -gX + nu; an instance stops after a pass with max |dx_k[i]| over its active rows
   <= SX17_EQ max(1, |dx|_inf), otherwise nu += rho dx on those rows; SX17_ITERS passes without
   that: status 2 (MPCB_STATUS_MAXITER) and the last pass's outputs.

``sbox_case`` restates the state-box draws of tests/test_gpu_full17.py (``_sbox_inputs``, seed 41,
iterate mode) and adds the oracle's solve, both masks by tolerance and cotangents.
"""
import functools
import json
import os

import numpy as np

from oracle.full import FullSpec, mpc_solve17
from oracle.ocp import riccati_solve

import vjp17_ref as vr
from vjp_weights_ref import _sym

SX17_RHO, SX17_EQ, SX17_ITERS = 1e8, 1e-10, 12   # mpcb_full.h (tests/test_vjp17x_ref_cpu.py compares)
KEYS, WKEYS = vr.KEYS, vr.WKEYS
# The bound of the device against ``dense_x``: 10 x the worst error of ``al_x`` against it over the
# short cases (2.3e-8), fixed and re-measured by tests/test_vjp17x_ref_cpu.py
SX_BOUND = 2.3e-7


def _mask_x(fixed_x, B, N):
    """bool [B,N+1,17] with stages 0 and N cleared (they are never read)."""
    m = np.zeros((B, N + 1, 17), dtype=bool) if fixed_x is None else np.asarray(fixed_x).astype(bool).copy()
    m[:, 0] = False
    m[:, N] = False
    return m


def _outputs_x(A, dx, du, gX, mu, spec):
    B, N = du.shape[:2]
    s = spec.s
    Q, R, QN = (np.asarray(M, dtype=np.float64) for M in (spec.Q, spec.R, spec.QN))
    gxref = np.empty_like(dx)
    gxref[:, :N] = s * np.einsum('ij,bkj->bki', Q, dx[:, :N])
    gxref[:, N] = np.einsum('ij,bj->bi', QN, dx[:, N])
    guref = s * np.einsum('ij,bkj->bki', R, du)
    nu_ = gX[:, N] - gxref[:, N]
    for k in range(N - 1, -1, -1):
        nu_ = gX[:, k] - gxref[:, k] - mu[:, k] + np.einsum('bji,bj->bi', A[:, k], nu_)
    return nu_, gxref, guref


def _weights(out, dx, du, X, U, xref, uref, spec):
    N = du.shape[1]
    rx = np.asarray(X, dtype=np.float64) - np.broadcast_to(np.asarray(xref, dtype=np.float64), dx.shape)
    ru = np.asarray(U, dtype=np.float64) - np.broadcast_to(np.asarray(uref, dtype=np.float64), du.shape)
    out.update(gQ=-spec.s * _sym(np.einsum('bki,bkj->bij', dx[:, :N], rx[:, :N])),
               gR=-spec.s * _sym(np.einsum('bki,bkj->bij', du, ru)),
               gQN=-_sym(np.einsum('bi,bj->bij', dx[:, N], rx[:, N])))


def _prep(xbar, ubar, p, fixed, fixed_x, gX, gU, spec):
    xbar, ubar = np.asarray(xbar, dtype=np.float64), np.asarray(ubar, dtype=np.float64)
    B, N = ubar.shape[:2]
    gX = np.zeros_like(xbar) if gX is None else np.asarray(gX, dtype=np.float64)
    gU = np.zeros_like(ubar) if gU is None else np.asarray(gU, dtype=np.float64)
    fixed = np.zeros((B, N, 6), dtype=bool) if fixed is None else np.asarray(fixed).astype(bool)
    A, Bm = vr.linearise17(xbar, ubar, p, spec)
    return A, Bm, fixed, _mask_x(fixed_x, B, N), gX, gU


def dense_x(xbar, ubar, p, fixed, fixed_x, gX, gU, spec, X=None, U=None, xref=None, uref=None):
    """dict(gx0, gxref, guref, dx, du, mu); with ``X``, ``U``, ``xref``, ``uref`` also gQ, gR, gQN."""
    A, Bm, fixed, mx, gX, gU = _prep(xbar, ubar, p, fixed, fixed_x, gX, gU, spec)
    B, N, nx, nu = Bm.shape
    s = spec.s
    Q, R, QN = (np.asarray(M, dtype=np.float64) for M in (spec.Q, spec.R, spec.QN))
    S = np.zeros((B, N + 1, nx, N, nu))   # dx_k = S_k du
    for k in range(N):
        S[:, k + 1] = np.einsum('bij,bjlm->bilm', A[:, k], S[:, k])
        S[:, k + 1, :, k] = Bm[:, k]
    S = S.reshape(B, N + 1, nx, N * nu)
    H = np.zeros((B, N * nu, N * nu))
    g = gU.reshape(B, N * nu).copy()
    for k in range(N + 1):
        Wk = s * Q if k < N else QN
        H += np.matmul(np.swapaxes(S[:, k], 1, 2), np.matmul(Wk[None], S[:, k]))
        g += np.einsum('bij,bi->bj', S[:, k], gX[:, k])
    for k in range(N):
        H[:, k * nu:(k + 1) * nu, k * nu:(k + 1) * nu] += s * R
    fx = fixed.reshape(B, N * nu)
    fr = fx[:, :, None] | fx[:, None, :]
    H = np.where(fr, 0.0, H) + np.einsum('bi,ij->bij', fx.astype(np.float64), np.eye(N * nu))
    g = np.where(fx, 0.0, g)
    dxs, dus, mus = np.zeros((B, N + 1, nx)), np.zeros((B, N, nu)), np.zeros((B, N + 1, nx))
    for b in range(B):   # (the row count differs by instance)
        ks, is_ = np.nonzero(mx[b])
        C = np.where(fx[b][None, :], 0.0, S[b, ks, is_, :])   # a clamped input is no unknown
        m = C.shape[0]
        KKT = np.zeros((N * nu + m, N * nu + m))
        KKT[:N * nu, :N * nu] = H[b]
        KKT[:N * nu, N * nu:] = C.T
        KKT[N * nu:, :N * nu] = C
        sol = np.linalg.lstsq(KKT, np.concatenate([g[b], np.zeros(m)]), rcond=None)[0]
        dus[b] = sol[:N * nu].reshape(N, nu)
        mus[b, ks, is_] = sol[N * nu:]
        dxs[b] = np.einsum('kij,j->ki', S[b], sol[:N * nu])
    out = dict(zip(KEYS, _outputs_x(A, dxs, dus, gX, mus, spec)), dx=dxs, du=dus, mu=mus)
    if X is not None:
        _weights(out, dxs, dus, X, U, xref, uref, spec)
    return out


def al_x(xbar, ubar, p, fixed, fixed_x, gX, gU, spec, X=None, U=None, xref=None, uref=None, rho=SX17_RHO,
         eq_tol=SX17_EQ, iters=SX17_ITERS):
    """dict(gx0, gxref, guref, dx, du, status [B] int32 (0, 2 = not converged, 4 = QP failure),
    passes [B], eq [B] (the last pass's residual)); with ``X`` ... also gQ, gR, gQN."""
    A, Bm, fixed, mx, gX, gU = _prep(xbar, ubar, p, fixed, fixed_x, gX, gU, spec)
    B, N, nx, nu = Bm.shape
    zx, zu = np.zeros((B, N + 1, nx)), np.zeros((B, N, nu))
    xref_t = zx.copy()   # p_N = QN (0 - xref_N) = -gX_N (tests/vjp_ref.py _riccati)
    xref_t[:, N] = np.linalg.solve(np.asarray(spec.QN, dtype=np.float64), gX[:, N].T).T
    nu_ = np.zeros((B, N + 1, nx))
    done = np.zeros(B, dtype=bool)
    okall = np.ones(B, dtype=bool)
    passes = np.zeros(B, dtype=np.int32)
    eqs = np.zeros(B)
    dxo, duo, muo = zx.copy(), zu.copy(), zx.copy()
    mxf = mx.astype(np.float64)
    for _ in range(iters):
        dx, du, _, ok = riccati_solve(A, Bm, zx[:, :N], np.zeros((B, nx)), zx, zu, xref_t, zu, spec, fixed=fixed,
                                      delta=zu, Rd=zu, rd=-gU, Qd=rho * mxf[:, :N], qd=-gX[:, :N] + nu_[:, :N])
        run = ~done
        dxo[run], duo[run] = dx[run], du[run]
        muo[run] = (nu_ + rho * mxf * dx)[run]   # the multipliers of this pass's subproblem
        passes[run] += 1
        okall &= ok
        eq = np.abs(dx * mxf).max(axis=(1, 2))
        dm = np.abs(dx).max(axis=(1, 2))
        eqs[run] = eq[run]
        done |= (eq <= eq_tol * np.maximum(1.0, dm)) | ~ok
        if done.all():
            break
        upd = ~done
        nu_[upd] += rho * (mxf * dx)[upd]
    out = dict(zip(KEYS, _outputs_x(A, dxo, duo, gX, muo, spec)), dx=dxo, du=duo,
               status=np.where(~okall, 4, np.where(done, 0, 2)).astype(np.int32), passes=passes, eq=eqs)
    if X is not None:
        _weights(out, dxo, duo, X, U, xref, uref, spec)
    return out


def random_mask_x(B, N, frac, seed=9):
    """A synthetic set of active state rows: about ``frac`` of the rows, stages 0 and N cleared."""
    m = np.random.default_rng(seed).random((B, N + 1, 17)) < frac
    m[:, 0] = False
    m[:, N] = False
    return m


SYNTH = {(5, 3): 0.08, (7, 17): 0.05, (3, 60): 0.03}   # shape of vr.vjp17_case -> frac of random_mask_x


def synth_case(B, N):
    """(case, fixed, fixed_x) of the synthetic-mask tests on an unboxed handle."""
    return vr.vjp17_case(B, N), vr.random_mask(B, N, frac=0.3), random_mask_x(B, N, SYNTH[(B, N)])


def state_box():
    d = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ocp_json_pin.json')))
    return np.array(d['lbx']), np.array(d['ubx'])


def sbox_inputs(B, N, seed=41):
    """The state-box draws of tests/test_gpu_full17.py in iterate mode."""
    lbx, ubx = state_box()
    x0, xref, uref, p = vr.inputs17(B, N, seed)
    rng = np.random.default_rng(seed + 1)
    x0 = rng.uniform(0.25 * lbx, 0.25 * ubx, (B, 17))
    x0[:, 2] = 3.5 + rng.uniform(-0.5, 0.5, B)
    rng = np.random.default_rng(seed + 1)
    xbar = x0[:, None, :] + rng.normal(0, 0.01, (B, N + 1, 17))
    ubar = uref + rng.normal(0, 0.5, (B, N, 6))
    return dict(x0=x0, xref=xref, uref=uref, p=p, xbar=xbar, ubar=ubar), lbx, ubx


def state_mask(X, lbx, ubx, tol=vr.ACTIVE_TOL):
    """Active state rows by tolerance (slack < tol on stages 1..N-1), and the slack of every row."""
    slack = np.minimum(X - lbx, ubx - X)
    m = slack < tol
    m[:, 0] = False
    m[:, -1] = False
    return m, slack


@functools.lru_cache(maxsize=None)
def sbox_case(B, N):
    """The end-to-end case: (spec, c) with c the inputs, the oracle's solve ``o``, ``fixed`` / ``fixed_x``
    by tolerance from it and cotangents gX, gU from default_rng(7).  Read-only, shared."""
    c, lbx, ubx = sbox_inputs(B, N)
    spec = FullSpec(N=N, lbu=vr.LBU17, ubu=vr.UBU17, lbx=lbx, ubx=ubx)
    o = mpc_solve17(c['x0'], c['xref'], c['uref'], spec, c['p'], mode='iterate', xbar=c['xbar'], ubar=c['ubar'])
    rng = np.random.default_rng(7)
    c.update(o=o, fixed=vr.active_mask(o['U'], spec)[0], fixed_x=state_mask(o['X'], lbx, ubx)[0],
             gX=rng.standard_normal((B, N + 1, 17)), gU=rng.standard_normal((B, N, 6)), lbx=lbx, ubx=ubx)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return spec, c


# ---------------------------------------------------------------------- the directional tests
FD_H, FD_SEED = 1e-4, 13   # tests/test_vjp17x_ref_cpu.py: the masks of the (5, 12) draw hold at +-h


def fd_direction(B, N):
    """The direction of the central-difference tests in (x0, xref, uref)."""
    rng = np.random.default_rng(FD_SEED)
    return rng.standard_normal((B, 17)), rng.standard_normal((B, N + 1, 17)), rng.standard_normal((B, N, 6))


# ---------------------------------------------------------------------- the closed loop with the state box
LOOP_B, LOOP_N, LOOP_NSIM = 3, 8, 2


def loop_ref(c, spec, x0=None, xref=None, uref=None):
    """The loop of closed_loop_diff(warm_start=False) by the oracle: every step solves at the given
    (xbar, ubar), the plant applies u0 under the controller's parameters.  Returns X_sim [B,nsim+1,17],
    U_sim [B,nsim,6], the per-step solves' (X, U), their masks and statuses."""
    from oracle.full import rk4_step17
    x = np.array(c['x0'] if x0 is None else x0, dtype=np.float64)
    xref = c['xref'] if xref is None else xref
    uref = c['uref'] if uref is None else uref
    Xs, Us, steps = [x], [], []
    for _ in range(LOOP_NSIM):
        o = mpc_solve17(x, xref, uref, spec, c['p'], mode='iterate', xbar=c['xbar'], ubar=c['ubar'])
        steps.append(dict(status=o['status'], fixed=vr.active_mask(o['U'], spec)[0],
                          fixed_x=state_mask(o['X'], spec.lbx, spec.ubx)[0]))
        u0 = o['U'][:, 0]
        x = rk4_step17(x, u0, c['p'], spec.dt, spec.params)
        Xs.append(x)
        Us.append(u0)
    return np.stack(Xs, axis=1), np.stack(Us, axis=1), steps


@functools.lru_cache(maxsize=None)
def loop_case():
    """The state-box draws at (LOOP_B, LOOP_N), loss weights w [B,nsim+1,17] from default_rng(23), and the
    gradient of sum(w X_sim) with respect to (x0, xref, uref) chained from the references alone:
    ``simvjp17_ref`` for the plant, ``dense_x`` on each solve's masks for the controller.  A solve whose
    product does not converge in ``al_x`` (``ok`` [nsim, B] False: instance 1 at step 0, a nearly
    dependent active set with rows 6e-7 off their bounds) passes no gradient, as in the torch layer."""
    from simvjp17_ref import simvjp17_ref
    B, N = LOOP_B, LOOP_N
    c, lbx, ubx = sbox_inputs(B, N)
    spec = FullSpec(N=N, lbu=vr.LBU17, ubu=vr.UBU17, lbx=lbx, ubx=ubx)
    w = np.random.default_rng(23).standard_normal((B, LOOP_NSIM + 1, 17))
    X, U, steps = loop_ref(c, spec)
    g = dict(xref=np.zeros_like(c['xref']), uref=np.zeros_like(c['uref']))
    lam = w[:, LOOP_NSIM].copy()
    ok = np.ones((LOOP_NSIM, B), dtype=bool)
    for i in reversed(range(LOOP_NSIM)):
        o = simvjp17_ref(X[:, i], U[:, i], lam, spec.dt, spec.params, c['p'])
        gU = np.zeros((B, N, 6))
        gU[:, 0] = o['gu']
        args = (c['xbar'], c['ubar'], c['p'], steps[i]['fixed'], steps[i]['fixed_x'], None, gU, spec)
        r = dense_x(*args)
        ok[i] = al_x(*args)['status'] == 0
        g['xref'] += np.where(ok[i][:, None, None], r['gxref'], 0.0)
        g['uref'] += np.where(ok[i][:, None, None], r['guref'], 0.0)
        lam = w[:, i] + o['gx'] + np.where(ok[i][:, None], r['gx0'], 0.0)
    g['x0'] = lam
    return dict(c=c, spec=spec, w=w, X=X, U=U, steps=steps, grad=g, ok=ok)
