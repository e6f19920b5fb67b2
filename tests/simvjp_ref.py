"""NumPy references of mpcb_sim_step_vjp (include/mpcb.h) and of the forward pass of
``closed_loop_diff``; a helper, not a test.

``simvjp_ref`` differentiates the discrete RK4 step x_out = Phi_b(x, u) of tests/pm_ref.py
``pm_sim_ref`` in FORWARD mode and applies the transpose to the cotangent:
 * gx = A^T g, gu = B^T g with (A, B) of ``oracle.rk4.rk4_sens`` at instance b's ``Params``;
 * gwind, gmodel from the parameter sensitivity S = d x_out / d theta, theta = (record, wind),
   propagated through the four stages with ``oracle.model.jac12`` as the state part,
       dk_1 = F(X_1),  dk_i = J_x(X_i) c_i h dk_{i-1} + F(X_i),  S = h/6 (dk_1 + 2 dk_2 + 2 dk_3 + dk_4),
   and F = d f / d theta written out below (``dfdtheta``) with Jinv as a function of J:
   d Jinv = -Jinv dJ Jinv, the nine entries of J independent.
The device runs reverse mode from captured scalars; nothing of that is shared here.
tests/test_simvjp_ref_cpu.py ties this reference to central differences of ``oracle.rk4.rk4_step``.

``loop_ref`` is the closed loop of ``closed_loop_diff`` (values only): per step ``pm_solve_ref`` with the
per-instance weights, then ``pm_sim_ref`` with the plant's vehicles.
"""
import numpy as np

from oracle.model import f12, jac12
from oracle.rk4 import rk4_sens

from pm_ref import MODEL_REC, params_of, pm_sim_ref, pm_solve_ref
from pw_ref import _row

NTH = MODEL_REC + 3   # record entries, then the wind


def dfdtheta(x, u, P, wind):
    """d f12 / d theta [12, 17] at one instance (x [12], u [4], wind [3])."""
    F = np.zeros((12, NTH))
    phi, th, psi = x[3], x[4], x[5]
    om = x[9:12]
    cf, sf, ct, st, cp, sp = np.cos(phi), np.sin(phi), np.cos(th), np.sin(th), np.cos(psi), np.sin(psi)
    re3 = np.array([cp * cf * st + sp * sf, sp * cf * st - cp * sf, cf * ct])
    Ttot = u.sum() + P.t_blast
    # v_dot = (re3 Ttot + wind) / mass - g e3
    F[6:9, 0] = -(re3 * Ttot + wind) / P.mass ** 2
    F[6:9, 4] = re3 / P.mass
    F[6:9, MODEL_REC:] = np.eye(3) / P.mass
    # omega_dot = Jinv m,  m = Mom(u) - om x J om
    J = np.asarray(P.J, dtype=np.float64)
    Ji = np.linalg.inv(J)
    d = np.array([u[1] + u[3] - u[0] - u[2], u[1] + u[2] - u[0] - u[3], u[2] + u[3] - u[0] - u[1]])
    m = d * np.array([P.ly, P.lx, P.c]) - np.cross(om, J @ om)
    F[9:12, 1] = Ji[:, 1] * d[1]   # lx
    F[9:12, 2] = Ji[:, 0] * d[0]   # ly
    F[9:12, 3] = Ji[:, 2] * d[2]   # c
    for i in range(3):
        for j in range(3):
            E = np.zeros((3, 3))
            E[i, j] = 1.0
            F[9:12, 5 + 3 * i + j] = -Ji @ E @ Ji @ m - Ji @ np.cross(om, E @ om)
    return F


def _one(x, u, g, T, P, wind):
    w = np.zeros(3) if wind is None else wind
    _, A, Bm = rk4_sens(x[None], u[None], T, P, None if wind is None else wind[None])
    gx, gu = A[0].T @ g, Bm[0].T @ g
    f = lambda xs: f12(xs[None], u[None], P, w[None])[0]   # noqa: E731
    Jx = lambda xs: jac12(xs[None], u[None], P, w[None])[0][:, :12]   # noqa: E731
    k1, d1 = f(x), dfdtheta(x, u, P, w)
    x2 = x + 0.5 * T * k1
    k2, d2 = f(x2), Jx(x2) @ (0.5 * T * d1) + dfdtheta(x2, u, P, w)
    x3 = x + 0.5 * T * k2
    k3, d3 = f(x3), Jx(x3) @ (0.5 * T * d2) + dfdtheta(x3, u, P, w)
    x4 = x + T * k3
    d4 = Jx(x4) @ (T * d3) + dfdtheta(x4, u, P, w)
    S = (T / 6.0) * (d1 + 2.0 * d2 + 2.0 * d3 + d4)
    gth = S.T @ g
    return gx, gu, gth[MODEL_REC:], gth[:MODEL_REC]


def simvjp_ref(x, u, gxn, T, spec, models=None, wind=None):
    """dict(gx [B,12], gu [B,4], gwind [B,3], gmodel [B,14]) of the step of length T of instance b's
    vehicle (``models`` [B|1, 14]; None = the spec's) under ``wind`` ([B|1, 3] or None = 0)."""
    from pm_ref import pack_params
    x, u, gxn = (np.asarray(a, dtype=np.float64) for a in (x, u, gxn))
    B = x.shape[0]
    models = np.asarray(pack_params(spec.params)[None] if models is None else models, dtype=np.float64)
    outs = []
    for b in range(B):
        P = params_of(models[b if models.shape[0] > 1 else 0], spec.params)
        w = _row(wind, b, B)
        outs.append(_one(x[b], u[b], gxn[b], T, P, None if w is None else w[0]))
    return {k: np.stack([o[i] for o in outs]) for i, k in enumerate(('gx', 'gu', 'gwind', 'gmodel'))}


def loop_ref(x0, xref, uref, nsim, xbar, ubar, spec, Q=None, R=None, QN=None, plant_models=None, wind=None,
             plant_T=None, warm_start=True):
    """(X_sim [B, nsim+1, 12], U_sim [B, nsim, 4], status [B] = max over steps, fixed [B, nsim, N, 4]) of
    ``closed_loop_diff``'s forward pass; ``fixed`` is every solve's active set (all False without a box).
    Q, R, QN: [B|1, n, n] or None.  warm_start: the next step linearises at this step's (X, U)."""
    from vjp_ref import active_set
    x = np.asarray(x0, dtype=np.float64).copy()
    B, N = x.shape[0], spec.N
    xb, ub = np.array(xbar, dtype=np.float64), np.array(ubar, dtype=np.float64)
    T = spec.dt if plant_T is None else plant_T
    Xs, Us = np.empty((B, nsim + 1, 12)), np.empty((B, nsim, 4))
    fixed = np.zeros((B, nsim, N, 4), dtype=bool)
    worst = np.zeros(B, dtype=np.int32)
    Xs[:, 0] = x
    for i in range(nsim):
        r = pm_solve_ref(x, xref, uref, xb, ub, spec, None, Q, R, QN, wind)
        worst = np.maximum(worst, r['status'].astype(np.int32))
        a = active_set(r['U'], spec)
        if a is not None:
            fixed[:, i] = a
        if warm_start:
            xb, ub = r['X'], r['U']
        Us[:, i] = r['u0']
        x = pm_sim_ref(x, r['u0'], T, spec, plant_models, wind)
        Xs[:, i + 1] = x
    return Xs, Us, worst, fixed


# ------------------------------------------------------------------ the frozen closed-loop case
# Shared by tests/test_simvjp_ref_cpu.py (which asserts its conditions) and tests/test_gpu_simvjp.py.
LOOP_B, LOOP_N, LOOP_NSIM, LOOP_SEED, LOOP_NDIR = 3, 3, 3, 14, 4
LOOP_LB, LOOP_UB = np.full(4, 5.0), np.full(4, 40.0)   # the box of tests/test_pm_ref_cpu.py box_case
LOOP_STEPS = (1e-3, 5e-4, 2.5e-4)   # the quotients use the first pair; the second pair measures them
# the Richardson self-agreement of the quotients as tests/test_simvjp_ref_cpu.py measured it (boxed: True),
# and the bound it holds them to; tests/test_gpu_simvjp.py allows max(1e-9, 10 x the recorded figure)
LOOP_SELF = {True: 3.7e-11, False: 9.2e-11}
LOOP_SELF_BOUND = 1e-9
LOOP_KEYS = ('x0', 'xref', 'uref', 'Q', 'R', 'QN', 'plant_model')


def loop_case(box=True):
    """The frozen case (never modified by its users): spec, the point theta (a dict over LOOP_KEYS,
    Q / R / QN as diagonals [B, n]), xbar / ubar, the loss weights w [B, nsim+1, 12] and LOOP_NDIR
    directions (dicts like theta).  x0 is hover moved by N(0, 1) (0.6 m in position, 0.3 m/s in
    velocity, 0.05 in the angles and rates), which drives some u0 component onto the box [5, 40];
    weights and vehicles are the draws of pw_weights / pm_models (dense J).  A direction is N(0, 1)
    times 0.1 for x0 and xref, 1 for uref, and |entry| for the weights and the vehicle records, which
    keeps every weight positive at the steps of LOOP_STEPS."""
    from oracle.ocp import OcpSpec
    from pm_ref import pm_models
    from pw_ref import pw_weights
    from vjp_ref import vjp_case
    B, N = LOOP_B, LOOP_N
    spec = OcpSpec(N=N, lbu=LOOP_LB if box else None, ubu=LOOP_UB if box else None)
    c = vjp_case(B, N, spec, 'sine')
    rng = np.random.default_rng(LOOP_SEED)
    x0 = c['x0'] + rng.standard_normal((B, 12)) * np.repeat([0.6, 0.05, 0.3, 0.05], 3)
    Q, R, QN = pw_weights(B, spec)
    dg = lambda W: np.stack([np.diag(M) for M in W])   # noqa: E731
    th = dict(x0=x0, xref=c['xref'].copy(), uref=c['uref'].copy(), Q=dg(Q), R=dg(R), QN=dg(QN),
              plant_model=pm_models(B, spec))
    w = rng.standard_normal((B, LOOP_NSIM + 1, 12))
    scale = dict(x0=0.1, xref=0.1, uref=1.0, Q=np.abs(th['Q']), R=np.abs(th['R']), QN=np.abs(th['QN']),
                 plant_model=np.abs(th['plant_model']))
    dirs = [{k: rng.standard_normal(th[k].shape) * scale[k] for k in LOOP_KEYS} for _ in range(LOOP_NDIR)]
    return dict(spec=spec, theta=th, xbar=c['xbar'].copy(), ubar=c['ubar'].copy(), w=w, dirs=dirs)


def loop_eval(case, theta):
    """loop_ref at theta with warm_start=False: (loss = sum w X_sim, X_sim, U_sim, status, fixed)."""
    de = lambda D: np.stack([np.diag(v) for v in D])   # noqa: E731
    X, U, st, fixed = loop_ref(theta['x0'], theta['xref'], theta['uref'], LOOP_NSIM, case['xbar'], case['ubar'],
                               case['spec'], de(theta['Q']), de(theta['R']), de(theta['QN']),
                               theta['plant_model'], warm_start=False)
    return float((case['w'] * X).sum()), X, U, st, fixed


def loop_quotients(case, steps=LOOP_STEPS[:2]):
    """Per direction: the Richardson-extrapolated central quotient of the loss over the two relative
    steps, and whether every +- point had the active sets of the centre."""
    th = case['theta']
    fixed0 = loop_eval(case, th)[4]
    out, same = [], True
    for d in case['dirs']:
        q = []
        for h in steps:
            lp = loop_eval(case, {k: th[k] + h * d[k] for k in LOOP_KEYS})
            lm = loop_eval(case, {k: th[k] - h * d[k] for k in LOOP_KEYS})
            same = same and np.array_equal(lp[4], fixed0) and np.array_equal(lm[4], fixed0)
            same = same and not lp[3].any() and not lm[3].any()
            q.append((lp[0] - lm[0]) / (2.0 * h))
        out.append((4.0 * q[1] - q[0]) / 3.0)
    return np.array(out), same
