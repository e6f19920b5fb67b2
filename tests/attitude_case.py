"""Attitude draws for the parity tests over the full heading circle and flying tilt; a helper, not
a test.  Pure NumPy, seeded.

The draws of the rest of the suite keep roll and pitch within +-0.17 rad and yaw within +-0.35 rad,
where the quadrant index n = rint(a 2/pi) of the hand-written sin/cos (mpcb_model.h sc_core) is 0
and the terms of the trig consumers that sin(phi), sin(theta), sin(psi) and tan(theta) multiply
are small.  Three groups of per-instance attitude offsets [B, 3] (roll, pitch, yaw) leave that slab;
they are added to the Euler angles of a base draw (``apply``), b is the instance index:

 H  heading: yaw offset wrap((pi/2)(b mod 4) + U(-pi/4, pi/4)), nothing else.  The QPs stay as
    benign as the base draw's (yaw enters the dynamics through a rotation about the thrust axis).
 T  tilt: H plus roll and pitch offsets s U(0.6, 1.0) with independent random signs s: n in
    {-1, 0, 1} for both and cos(theta) >= 0.4.
 I  any attitude: roll and yaw by the H formula with different residues; pitch *set* to s U(0, 1.26)
    on half of the instances and to s (pi - U(0, 1.26)) on the other half: |cos(theta)| >= 0.3 with
    |theta| > pi/2 included.

``swivel`` draws the 17/6 model's swivel angles over the reference's own state box:
alpha1 = U(-0.17, 1.22), alpha2 = U(-0.52, 0.52).

``apply(x, d)`` adds the offsets to x[..., 3:6] of a state [B, 12 | 17] or a trajectory
[B | 1, N + 1, 12 | 17] (a broadcast row is expanded to B rows).  ``place=True`` sets roll and
pitch to the offsets instead: for base draws that spread the angles themselves widely (the plant
step's x in U(-0.5, 0.5)), where a sum would leave the cos(theta) floor, and for the pitch of I.

The case builders below put the offsets on the base draws of the existing tests (reused, not
copied).  In cases built like ``vjp_case`` the offset goes on x0 before the rollout that makes
xbar: the base case is drawn once, its noise on xbar and x0 is recovered as the difference to its
own rollout, and the rollout is repeated from the turned x0.
"""
import functools

import numpy as np

GROUPS = ('H', 'T', 'I')
SEED = {'H': 2102, 'T': 2101, 'I': 2106}   # chosen on the reference alone: tests/test_attitude_case_cpu.py
CASE17_SEED = 1708   # the base draw of the 17/6 entry-point cases (B = 13): see case17
STEP17_SEED = {'H': 2102, 'T': 2200, 'I': 2201}
COS_FLOOR = {'H': 0.85, 'T': 0.4, 'I': 0.3}   # |cos(theta)| along a case's trajectories (H: the base draws')


def wrap(a):
    return (np.asarray(a, dtype=np.float64) + np.pi) % (2.0 * np.pi) - np.pi


def quadrant(a):
    """n = rint(a 2/pi), the quadrant index of sc_core's reduction."""
    return np.rint(np.asarray(a, dtype=np.float64) * (2.0 / np.pi)).astype(np.int64)


def _circle(rng, residue):
    return wrap(0.5 * np.pi * (residue % 4) + rng.uniform(-np.pi / 4, np.pi / 4, residue.shape[0]))


def offsets(group, B, seed=None):
    """[B, 3] roll, pitch and yaw offsets of ``group`` ('H', 'T', 'I'; a trailing '17' is ignored)."""
    g = group[0]
    rng = np.random.default_rng(SEED[g] if seed is None else seed)
    b = np.arange(B)
    d = np.zeros((B, 3))
    d[:, 2] = _circle(rng, b)
    if g == 'T':
        d[:, :2] = rng.choice([-1.0, 1.0], (B, 2)) * rng.uniform(0.6, 1.0, (B, 2))
    elif g == 'I':
        d[:, 0] = _circle(rng, b + b // 4 + 1)
        t = rng.uniform(0.0, 1.26, B)
        d[:, 1] = rng.choice([-1.0, 1.0], B) * np.where((b // 2) % 2 == 1, np.pi - t, t)
    d.setflags(write=False)
    return d


def swivel(B, seed=2117):
    """[B, 2] swivel angles alpha1, alpha2 of the 17/6 model."""
    rng = np.random.default_rng(seed)
    a = np.stack([rng.uniform(-0.17, 1.22, B), rng.uniform(-0.52, 0.52, B)], axis=1)
    a.setflags(write=False)
    return a


def apply(x, d, place=False, pitch=False):
    """A copy of ``x`` with the offsets on its Euler angles.  ``place``: roll and pitch are set to
    the offsets; ``pitch``: the pitch alone is set (group I)."""
    x = np.asarray(x, dtype=np.float64)
    B = d.shape[0]
    dd = d if x.ndim == 2 else d[:, None, :]
    out = np.array(np.broadcast_to(x, (B,) + x.shape[1:]))
    if place:
        out[..., 3:5] = 0.0
    elif pitch:
        out[..., 4] = 0.0
    out[..., 3:6] += dd
    return out


def _sets_pitch(group):
    return group[0] == 'I'


# ------------------------------------------------------------------------------ 12/4 solve paths
@functools.lru_cache(maxsize=None)
def solve_inputs(group, N, B, dtype):
    """tests/test_gpu_config.py ``_inputs`` (make_inputs('c3'), its iterate and its wind) with the
    group's offsets on x0, every stage of xref and of xbar."""
    import test_gpu_config as gc
    inp = dict(gc._inputs(N, B, 'f64'))
    d = offsets(group, B)
    for k in ('x0', 'xref', 'xbar'):
        inp[k] = apply(inp[k], d)
    c = gc._cast(dtype)
    return {k: c(v) for k, v in inp.items()}


def config(boxed, dtype, full=False):
    """The MPCConfig fields of the default problem definition: nothing, or the box [0, 65] (17/6:
    the reference's input box), as a handle of ``dtype`` holds them (tests/alt_config.py)."""
    import alt_config as ac
    return ac.fields(full=full, groups=(), box='input' if boxed else 'none', dtype=dtype)


def use_wind(mode, group):
    """test_gpu_config._use_wind's alternation, the groups in the place of its variants."""
    return (mode == 'iterate') != (group[0] == 'T')


@functools.lru_cache(maxsize=None)
def solve_oracle(group, N, B, mode, dtype, boxed, max_as_iter=200):
    """(oracle output with the linearisation, spec) of the default problem definition; boxed: [0, 65]."""
    from oracle.ocp import OcpSpec, mpc_solve
    inp = solve_inputs(group, N, B, dtype)
    spec = OcpSpec(N=N, max_as_iter=max_as_iter, **config(boxed, dtype))
    wind = inp['wind'] if use_wind(mode, group) else None
    it = dict(mode='iterate', xbar=inp['xbar'], ubar=inp['ubar']) if mode == 'iterate' else {}
    return mpc_solve(inp['x0'], inp['xref'], inp['uref'], spec, wind=wind, return_lin=True, **it), spec


# ------------------------------------------------------------------------------ 12/4 products, gains, pw, pm
@functools.lru_cache(maxsize=None)
def product_case(group, B, N, ref='hover', wind=False):
    """tests/vjp_ref.py ``vjp_case`` with the offsets on x0 before the rollout that makes xbar, and
    on every stage of xref; plus the per-instance weights and vehicles of the pw / pm tests."""
    from oracle.ocp import OcpSpec, rollout
    from pm_ref import pm_models
    from pw_ref import pw_weights
    from vjp_ref import vjp_case
    spec = OcpSpec(N=N)
    c = dict(vjp_case(B, N, spec, ref, wind))
    d = offsets(group, B)
    base = rollout(_vjp_x0(B), c['ubar'], spec, c['wind'])
    noise_bar, noise_0 = c['xbar'] - base, c['x0'] - _vjp_x0(B)
    x0 = apply(_vjp_x0(B), d)
    c['xbar'] = rollout(x0, c['ubar'], spec, c['wind']) + noise_bar
    c['x0'] = x0 + noise_0
    c['xref'] = apply(c['xref'], d)
    Q, R, QN = pw_weights(B, spec)
    c.update(Q=Q, R=R, QN=QN, M=pm_models(B, spec))
    for v in c.values():
        if v is not None:
            v.setflags(write=False)
    return c


def _vjp_x0(B):
    """vjp_case's x0 before its noise: hover + 0.1 (make_x0 - hover) of seed 1004."""
    from oracle.inputs import draws, hover_state, make_x0
    hov = hover_state()
    return hov + 0.1 * (make_x0(draws(1004, np.arange(B, dtype=np.uint64))) - hov)


# ------------------------------------------------------------------------------ 12/4 dynamics calls
@functools.lru_cache(maxsize=None)
def step_case(group, B):
    """The plant-step draw of tests/test_gpu_simvjp.py / tests/test_gpu_pm.py (seed 4: x in
    U(-0.5, 0.5), u in U(0, 65), wind in U(-2, 2), vehicles pm_models, cotangent N(0, 1)), roll and
    pitch set to the offsets (T, I) and the yaw offset added."""
    import test_gpu_simvjp as gs
    c = {k: v[:B] for k, v in gs._case().items()}
    c['x'] = apply(c['x'], offsets(group, B), place=group[0] != 'H')
    c['x'].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def lin_case(group, B, N):
    """Trajectories to linearise along: the eval case's X and U (below) and its wind."""
    x0, xref, uref, w, U, X = eval_case(group, B, N, True)
    return X, U, w


@functools.lru_cache(maxsize=None)
def eval_case(group, B, N, wind):
    """tests/test_gpu_eval.py ``_case12`` (sine references) with the offsets on x0 before its
    rollout and on xref: x0, xref [B, ...], uref [1, ...], wind, U, X."""
    import test_gpu_eval as ge
    from eval_ref import rollout_any
    x0, xref, uref, w, U, X = ge._case12(B, N, 'sine', wind)
    d = offsets(group, B)
    noise = X - rollout_any(x0, U, ge._spec12(N), w)
    x0 = apply(x0, d, pitch=_sets_pitch(group))
    xref = apply(xref, d, pitch=_sets_pitch(group))
    X = rollout_any(x0, U, ge._spec12(N), w) + noise
    for a in (x0, xref, X):
        a.setflags(write=False)
    return x0, xref, uref, w, U, X


# ------------------------------------------------------------------------------ 17/6
@functools.lru_cache(maxsize=None)
def case17(group, B, N, seed=1704):
    """tests/vjp17_ref.py ``vjp17_case`` (inputs17, stage-constant parameters) with the offsets and
    the swivel draw on x0 before the rollout that makes xbar, and on every stage of xref.  The solves
    keep that file's seed; the product and gains cases take CASE17_SEED: at seed 1704 the two fp64
    references of the product (Riccati and condensed dense) disagree by 4e-11 on instance 0 of the
    unturned base draw already, a rounding amplification of 4e5 that no fp32 kernel can hold to
    5e-4; 1708 is the first seed from there on at which they agree within 5e-4 x 2^-29 on H and T
    (tests/test_attitude_case_cpu.py)."""
    import vjp17_ref as vr
    from oracle.full import FullSpec
    spec = FullSpec(N=N)
    c = dict(vr.vjp17_case(B, N, spec, seed))
    d, a = offsets(group, B), swivel(B)
    noise = c['xbar'] - vr.rollout17(c['x0'], c['ubar'], c['p'], spec)
    x0 = apply(c['x0'], d, pitch=_sets_pitch(group))
    x0[:, 12:14] = a
    xref = apply(c['xref'], d, pitch=_sets_pitch(group))
    xref[..., 12:14] = a[:, None, :]
    c.update(x0=x0, xref=xref, xbar=vr.rollout17(x0, c['ubar'], c['p'], spec) + noise)
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def solve17_inputs(group, B, N, dtype):
    """x0, xref, uref, p, xbar, ubar of ``case17`` as a handle of ``dtype`` sees them."""
    import test_gpu_config as gc
    c = case17(group, B, N)
    return tuple(gc._cast(dtype)(c[k]) for k in ('x0', 'xref', 'uref', 'p', 'xbar', 'ubar'))


@functools.lru_cache(maxsize=None)
def solve17_oracle(group, B, N, mode, dtype, boxed):
    from oracle.full import FullSpec, mpc_solve17
    x0, xref, uref, p, xb, ub = solve17_inputs(group, B, N, dtype)
    spec = FullSpec(N=N, **config(boxed, dtype, full=True))
    it = dict(mode='iterate', xbar=xb, ubar=ub) if mode == 'iterate' else {}
    return mpc_solve17(x0, xref, uref, spec, p, **it), spec


@functools.lru_cache(maxsize=None)
def step17_case(group, B):
    """The plant-step draw of tests/simvjp17_ref.py ``step_case`` (x in U(-0.5, 0.5), ...), its first
    B instances, with roll and pitch set to the offsets (T, I), the yaw offset added and the swivel
    draw in x[12:14].  The offsets have seeds of their own (STEP17_SEED): that file measures each
    gradient block relative to its own largest entry, and at these seeds no instance's d/dT_blast
    falls under its REF_FLOOR (tests/test_attitude_case_cpu.py)."""
    import simvjp17_ref as s17
    c = {k: v[:B] for k, v in s17.step_case().items()}
    c['x'] = apply(c['x'], offsets(group, B, STEP17_SEED[group[0]]), place=group[0] != 'H')
    c['x'][:, 12:14] = swivel(B)
    for v in c.values():
        v.setflags(write=False)
    return c
