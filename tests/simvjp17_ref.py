"""NumPy references of mpcb_sim_step_vjp17 (include/mpcb.h) and of the forward pass of
``closed_loop_diff`` on the 17/6 model; a helper, not a test.

``simvjp17_ref`` differentiates the discrete RK4 step x_out = Phi(x, u; p) of ``oracle.full.rk4_step17``
in FORWARD mode and applies the transpose to the cotangent (the scheme of tests/simvjp_ref.py):
 * gx = A^T g, gu = B^T g with (A, B) of ``oracle.full.rk4_sens17`` (the complex step);
 * gparams from the parameter sensitivity S = d x_out / d p [17, 25], propagated through the four
   stages with ``oracle.full.jac17`` as the state part,
       dk_1 = F(X_1),  dk_i = J_x(X_i) c_i h dk_{i-1} + F(X_i),  S = h/6 (dk_1 + 2 dk_2 + 2 dk_3 + dk_4),
   and F = d f17 / d p written out below (``dfdp``).  ``oracle.model.unpack_params25`` casts to real,
   so a complex step in p does not work through the oracle.
The device runs reverse mode from captured scalars and takes the 24 Jacobian entries in closed form
(``closed_form``); nothing of that is shared with ``simvjp17_ref``.  tests/test_simvjp17_ref_cpu.py
ties this reference to central differences of ``rk4_step17`` and checks the closed form against it.

``loop17_ref`` is the closed loop of ``closed_loop`` / ``closed_loop_diff`` on the 17/6 model (values
only): per step ``oracle.full.mpc_solve17(mode='iterate')`` with the controller's parameters, then
``rk4_step17`` with the plant's, with every solve's active set from ``vjp17_ref.active_mask``.
"""
import numpy as np

from oracle.full import FullSpec, jac17, mpc_solve17, rk4_sens17, rk4_step17
from oracle.model import f17, rot_zyx

import vjp17_ref as vr

NP17 = 25
BLOCKS = ('gx', 'gu', 'gJ', 'gtb')   # the blocks of the metric: gJ = gparams[:24], gtb = gparams[24]


def dfdp(x, u, p, P):
    """d f17 / d p [17, 25] at one instance (x [17], u [6], p [25]; column-major blocks)."""
    F = np.zeros((17, NP17))
    fx = f17(x[None], u[None], p[None], P)[0]
    R = rot_zyx(x[3], x[4], x[5])
    s1, c1, s2, c2 = np.sin(x[12]), np.cos(x[12]), np.sin(x[13]), np.cos(x[13])
    F[6:9, 24] = R @ np.array([s1 * c2, -s2, c1 * c2]) / P.mass
    for i in range(3):
        for j in range(2):
            F[14 + i, j * 3 + i] = u[4 + j]        # J_angles[i][j] alpha_dot_j
        for j in range(3):
            F[14 + i, 6 + j * 3 + i] = fx[3 + j]   # J_euler[i][j] eta_dot_j
            F[14 + i, 15 + j * 3 + i] = x[6 + j]   # J_p[i][j] v_j
    return F


def _one(x, u, g, T, p, P):
    _, A, Bm = rk4_sens17(x[None], u[None], p[None], T, P)
    gx, gu = A[0].T @ g, Bm[0].T @ g
    f = lambda xs: f17(xs[None], u[None], p[None], P)[0]   # noqa: E731
    Jx = lambda xs: jac17(xs[None], u[None], p[None], P)[0][:, :17]   # noqa: E731
    k1, d1 = f(x), dfdp(x, u, p, P)
    x2 = x + 0.5 * T * k1
    k2, d2 = f(x2), Jx(x2) @ (0.5 * T * d1) + dfdp(x2, u, p, P)
    x3 = x + 0.5 * T * k2
    k3, d3 = f(x3), Jx(x3) @ (0.5 * T * d2) + dfdp(x3, u, p, P)
    x4 = x + T * k3
    d4 = Jx(x4) @ (T * d3) + dfdp(x4, u, p, P)
    S = (T / 6.0) * (d1 + 2.0 * d2 + 2.0 * d3 + d4)
    return gx, gu, S.T @ g


def simvjp17_ref(x, u, gxn, T, P, p):
    """dict(gx [B,17], gu [B,6], gparams [B,25]) of the step of length T under instance b's parameter
    vector (``p`` [B|1, 25] or [25])."""
    x, u, gxn = (np.asarray(a, dtype=np.float64) for a in (x, u, gxn))
    B = x.shape[0]
    p = np.broadcast_to(np.asarray(p, dtype=np.float64), (B, NP17))
    outs = [_one(x[b], u[b], gxn[b], T, p[b], P) for b in range(B)]
    return {k: np.stack([o[i] for o in outs]) for i, k in enumerate(('gx', 'gu', 'gparams'))}


def closed_form(x, u, gxn, T, P, p):
    """The 24 Jacobian entries of gparams [B,24] in the closed form the device uses: nothing reads
    the POC states, so gJp[i][c] = gxn[14+i] (x_out[c] - x[c]), gJe[i][c] = gxn[14+i] (x_out[3+c] - x[3+c]),
    gJa[i][c] = gxn[14+i] T u[4+c]."""
    x, u, gxn = (np.asarray(a, dtype=np.float64) for a in (x, u, gxn))
    B = x.shape[0]
    inc = rk4_step17(x, u, np.broadcast_to(np.asarray(p, dtype=np.float64), (B, NP17)), T, P) - x
    g = np.empty((B, 24))
    for i in range(3):
        for j in range(2):
            g[:, j * 3 + i] = gxn[:, 14 + i] * T * u[:, 4 + j]
        for j in range(3):
            g[:, 6 + j * 3 + i] = gxn[:, 14 + i] * inc[:, 3 + j]
            g[:, 15 + j * 3 + i] = gxn[:, 14 + i] * inc[:, j]
    return g


def blocks(out):
    """The four blocks of the metric from dict(gx, gu, gparams); keys absent from ``out`` are left out."""
    b = {k: out[k] for k in ('gx', 'gu') if k in out}
    if 'gparams' in out:
        b['gJ'], b['gtb'] = out['gparams'][:, :24], out['gparams'][:, 24:]
    return b


def blockerr(a, b):
    """Per instance |a - b|_inf / |b|_inf over the block: no floor of 1 (the parameter gradients are
    about 1e-2, which the project's floor would hide)."""
    a = np.asarray(a, dtype=np.float64).reshape(a.shape[0], -1)
    b = np.asarray(b, dtype=np.float64).reshape(b.shape[0], -1)
    return np.abs(a - b).max(axis=1) / np.abs(b).max(axis=1)


# ------------------------------------------------------------------ the frozen draw of the step tests
BMAX = 70   # one more than a 64-thread block: the last block is partial
SHAPES = (1, 5, BMAX)
REF_FLOOR = 1e-4   # every block of the frozen draw has |ref|_inf >= this (tests/test_simvjp17_ref_cpu.py)


def step_case(seed=11):
    """x in U(-0.5, 0.5), motor inputs in U(0, 65), swivel rates in U(-0.087, 0.087), p[:24] about
    0.3 N(0, 1), T_blast in U(10, 30), gxn in N(0, 1); BMAX instances.  Seed 11 is the first from 0 on at
    which every instance's d/dT_blast stays above REF_FLOOR for per-instance, broadcast and default
    parameters (a single entry per instance: some draw of 70 is small at most seeds)."""
    rng = np.random.default_rng(seed)
    u = np.concatenate([rng.uniform(0, 65, (BMAX, 4)), rng.uniform(-0.087, 0.087, (BMAX, 2))], axis=1)
    p = np.concatenate([0.3 * rng.standard_normal((BMAX, 24)), rng.uniform(10, 30, (BMAX, 1))], axis=1)
    return dict(x=rng.uniform(-0.5, 0.5, (BMAX, 17)), u=u, p=p, g=rng.standard_normal((BMAX, 17)))


# ------------------------------------------------------------------ the closed loop
def loop17_ref(x0, xref, uref, nsim, xbar, ubar, spec, p=None, plant_params=None, plant_T=None, warm_start=True,
               du=None):
    """(X_sim [B, nsim+1, 17], U_sim [B, nsim, 6], status [B] = max over steps, fixed [B, nsim, N, 6]).
    ``p``: the controller's parameters (None = the defaults); ``plant_params``: the plant's (None = p);
    ``du`` [B, nsim, 6]: added to the input the plant applies (the K of LOOP17_K), not to U_sim."""
    x = np.asarray(x0, dtype=np.float64).copy()
    B, N = x.shape[0], spec.N
    xb, ub = np.array(xbar, dtype=np.float64), np.array(ubar, dtype=np.float64)
    T = spec.dt if plant_T is None else plant_T
    pc = vr.stage_params(p, B, N)
    pp = np.broadcast_to(pc[:, 0] if plant_params is None else np.asarray(plant_params, dtype=np.float64), (B, NP17))
    Xs, Us = np.empty((B, nsim + 1, 17)), np.empty((B, nsim, 6))
    fixed = np.zeros((B, nsim, N, 6), dtype=bool)
    worst = np.zeros(B, dtype=np.int32)
    Xs[:, 0] = x
    for i in range(nsim):
        r = mpc_solve17(x, xref, uref, spec, pc, mode='iterate', xbar=xb, ubar=ub)
        worst = np.maximum(worst, r['status'].astype(np.int32))
        if spec.boxed:
            fixed[:, i] = vr.active_mask(r['U'], spec)[0]
        if warm_start:
            xb, ub = r['X'], r['U']
        Us[:, i] = r['u0']
        x = rk4_step17(x, r['u0'] if du is None else r['u0'] + du[:, i], pp, T, spec.params)
        Xs[:, i + 1] = x
    return Xs, Us, worst, fixed


# ------------------------------------------------------------------ the frozen closed-loop case
# Shared by tests/test_simvjp17_ref_cpu.py (which asserts its conditions) and tests/test_gpu_simvjp17.py.
LOOP17_B, LOOP17_N, LOOP17_NSIM, LOOP17_SEED, LOOP17_NDIR = 3, 3, 3, 11, 4
# the seed of the plant's parameters, the loss weights and the directions: the first from 111 on at which
# the boxed variant meets both conditions of tests/test_simvjp17_ref_cpu.py, found without the device:
#  * every +- point keeps the centre's active sets (at 111 and 112 a component of the last step's solve
#    sits 6e-3 off its bound and crosses it);
#  * the quotients agree with the reference's own adjoint (``loop17_grad_ref``) to LOOP17_GAP_BOUND.  The
#    oracle's interior point stops on the central path, where a weakly active component still moves with
#    the inputs, so the quotient of its loop differs from the derivative on the active set by 1e-10 to
#    1e-7 depending on the draw (113: 9.8e-9); a case for a 1e-9 check needs that gap well below 1e-9.
LOOP17_PSEED = 125
# the gap between quotient and reference adjoint as measured (boxed: True), and what the case is held to:
# a quarter of the 1e-9 bound of the GPU test
LOOP17_GAP = {True: 2.0e-10, False: 6.3e-11}
LOOP17_GAP_BOUND = 2.5e-10
LOOP17_STEPS = (1e-3, 5e-4, 2.5e-4)   # the quotients use the first pair; the second pair measures them
LOOP17_KEYS = ('x0', 'xref', 'uref', 'plant_params')
# the Richardson self-agreement of the quotients as tests/test_simvjp17_ref_cpu.py measured it (boxed:
# True) and the bound it holds them to; tests/test_gpu_simvjp17.py allows max(1e-9, 10 x the figure)
LOOP17_SELF = {True: 5.3e-11, False: 2.9e-11}
LOOP17_SELF_BOUND = 1e-7
# boxed: the move of the reference quotients per unit relative perturbation of the inputs the plant
# applies (``loop17_k``), as tests/test_simvjp17_ref_cpu.py measured it
LOOP17_K = 4.5
LOOP17_K_EPS = 1e-6


def loop17_case(box=True):
    """The frozen case (never modified by its users): ``vjp17_ref.boxed_case(3, 3, seed=11)`` with or
    without the reference's input box, plant_params = p (1 + 0.1 N(0, 1)), the loss weights
    w [B, nsim+1, 17] and LOOP17_NDIR directions (dicts over LOOP17_KEYS): N(0, 1) times 0.1 for x0 and
    xref, USCALE for uref and |entry| for plant_params."""
    B, N = LOOP17_B, LOOP17_N
    spec, c = vr.boxed_case(B, N, seed=LOOP17_SEED)
    if not box:
        spec = FullSpec(N=N)
    rng = np.random.default_rng(LOOP17_PSEED)
    pp = c['p'] * (1.0 + 0.1 * rng.standard_normal(c['p'].shape))
    th = dict(x0=c['x0'].copy(), xref=c['xref'].copy(), uref=c['uref'].copy(), plant_params=pp)
    w = rng.standard_normal((B, LOOP17_NSIM + 1, 17))
    scale = dict(x0=0.1, xref=0.1, uref=vr.USCALE, plant_params=np.abs(pp))
    dirs = [{k: rng.standard_normal(th[k].shape) * scale[k] for k in LOOP17_KEYS} for _ in range(LOOP17_NDIR)]
    return dict(spec=spec, theta=th, p=c['p'].copy(), xbar=c['xbar'].copy(), ubar=c['ubar'].copy(), w=w, dirs=dirs)


def loop17_eval(case, theta, du=None):
    """loop17_ref at theta with warm_start=False: (loss = sum w X_sim, X_sim, U_sim, status, fixed)."""
    X, U, st, fixed = loop17_ref(theta['x0'], theta['xref'], theta['uref'], LOOP17_NSIM, case['xbar'], case['ubar'],
                                 case['spec'], case['p'], theta['plant_params'], warm_start=False, du=du)
    return float((case['w'] * X).sum()), X, U, st, fixed


def loop17_quotients(case, steps=LOOP17_STEPS[:2], du=None):
    """Per direction: the Richardson-extrapolated central quotient of the loss over the two relative
    steps, and whether every +- point had status 0 and the active sets of the centre."""
    th = case['theta']
    fixed0 = loop17_eval(case, th, du)[4]
    out, same = [], True
    for d in case['dirs']:
        q = []
        for h in steps:
            lp = loop17_eval(case, {k: th[k] + h * d[k] for k in LOOP17_KEYS}, du)
            lm = loop17_eval(case, {k: th[k] - h * d[k] for k in LOOP17_KEYS}, du)
            same = same and np.array_equal(lp[4], fixed0) and np.array_equal(lm[4], fixed0)
            same = same and not lp[3].any() and not lm[3].any()
            q.append((lp[0] - lm[0]) / (2.0 * h))
        out.append((4.0 * q[1] - q[0]) / 3.0)
    return np.array(out), same


def loop17_grad_ref(case):
    """The gradient of loop17_eval's loss by the NumPy adjoints (warm_start=False): back through the
    steps with ``simvjp17_ref`` for the plant and ``vjp17_ref.vjp17_ref`` on each solve's active set for
    the controller.  A dict over LOOP17_KEYS.  What the device computes, from the references alone."""
    th, spec = case['theta'], case['spec']
    B, N, nsim = LOOP17_B, LOOP17_N, LOOP17_NSIM
    _, X, U, _, fixed = loop17_eval(case, th)
    g = dict(xref=np.zeros_like(th['xref']), uref=np.zeros_like(th['uref']), plant_params=np.zeros_like(th['plant_params']))
    lam = case['w'][:, nsim].copy()
    for i in reversed(range(nsim)):
        o = simvjp17_ref(X[:, i], U[:, i], lam, spec.dt, spec.params, th['plant_params'])
        g['plant_params'] += o['gparams']
        gU = np.zeros((B, N, 6))
        gU[:, 0] = o['gu']
        v = vr.vjp17_ref(case['xbar'], case['ubar'], case['p'], fixed[:, i] if spec.boxed else None, None, gU, spec)
        g['xref'] += v['gxref']
        g['uref'] += v['guref']
        lam = case['w'][:, i] + o['gx'] + v['gx0']
    g['x0'] = lam
    return g


def loop17_k(case, quot):
    """K: the largest move of a quotient, |q' - q| / max(|q|, 1), per unit of delta when the plant
    applies u0 + du with |du|_inf = delta max(|U_sim|_inf, 1) per instance (delta = LOOP17_K_EPS, seeded
    signs): the metric in which tests/test_gpu_simvjp17.py measures the device's U_sim against the
    oracle's."""
    U = loop17_eval(case, case['theta'])[2]
    rng = np.random.default_rng(LOOP17_PSEED + 100)
    den = np.maximum(np.abs(U).reshape(U.shape[0], -1).max(axis=1), 1.0)
    du = LOOP17_K_EPS * den[:, None, None] * rng.choice([-1.0, 1.0], size=U.shape)
    moved, _ = loop17_quotients(case, du=du)
    return float((np.abs(moved - quot) / np.maximum(np.abs(quot), 1.0)).max() / LOOP17_K_EPS)
