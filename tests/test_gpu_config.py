"""Every kernel path under a non-default problem definition.

The rest of the GPU suite varies shapes, batches, paths and precisions on ONE problem definition
(diagonal Q and R, QN = 10 Q, cost_scale == dt == 1/30, default mass / arms / gravity, the box
[0, 65] on every channel), which hides a transposed or mis-strided weight table, dt used where
cost_scale belongs, one channel's bound used for all, lbu treated as 0, or two model constants
swapped in one table.  Here ALT (tests/alt_config.py: dense SPD weights with QN no multiple of Q,
another mass, a general inertia, other arms, drag constant, gravity and blaster thrust, a
per-channel box with lbu != 0, and two dt / cost_scale variants of which ALT-b separates the two)
runs through every path of the 12/4 solve, the 17/6 solve, and linearize / sim_step / evaluate,
against the CPU oracle on identical inputs.  Conventions of tests/test_gpu_parity.py: fp32 inputs
and fp32 config values are rounded to fp32 before the oracle sees them; ``relerr`` is per instance
against max(|ref|, 1).

Bounds.  fp64 1e-9 on u0, X, U; fp32 5e-5 (N <= 40): the project's bounds against this oracle.
Statuses equal the oracle's and are all 0.  Box cases: per-channel feasibility within 1e-6 (fp64) /
2e-4 (fp32) of ALT's lbu / ubu, and in fp32 the rule of tests/test_gpu_fuzz.py: instances whose
exact minimiser moves by more than 1e-5 under fp32-level noise on [A|B] (oracle.ocp.fp32_sensitivity)
are held to the QP objective within 1e-5 instead, counted and printed (at most 5 % of a case).
17/6: the acceptance of tests/test_gpu_fuzz17.py with no OK-against-MINSTEP allowance.

Each case asserts the kernels it launched (``last_kernels() == plan_kernels(...)`` and the expected
names of its path), so a selection change cannot quietly empty a case, and asserts on the ORACLE's
output that the box is active (ALT-a, N = 6: >= 10 % of the input entries on a bound, at least one
instance through the interior point; 17/6: >= 20 %).  Each case prints its achieved errors
(DESIGN.md records the worst per path).
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alt_config as ac   # noqa: E402
from eval_ref import eval_ref, rollout_any   # noqa: E402

from oracle.full import FullSpec, mpc_solve17, rk4_sens17, rk4_step17   # noqa: E402
from oracle.inputs import draws, make_inputs, make_wind   # noqa: E402
from oracle.ocp import OcpSpec, fp32_sensitivity, mpc_solve, riccati_solve   # noqa: E402
from oracle.rk4 import rk4_sens, rk4_step   # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

B12 = 37          # nine full waves of four instances plus a ragged one
ON_BOUND = 1e-6   # an input entry of the oracle's U counts as on a bound within this
MODES = ('rollout', 'iterate')
ALTS = ('a', 'b')


def relerr(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(a.shape[0], -1)
    b = np.asarray(b, dtype=np.float64).reshape(b.shape[0], -1)
    return np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1.0)


def _cast(dtype):
    if dtype == 'f32':
        return lambda a: None if a is None else np.asarray(a, dtype=np.float32).astype(np.float64)
    return lambda a: a


def _it(mode):
    return 'true' if mode == 'iterate' else 'false'


# ------------------------------------------------------------------------------ 12/4 paths
# path -> (environment switches around handle creation, handle max_batch or None for the batch,
#          the kernels a solve launches on ALT (general inertia), by dtype letter and mode)
T = {'f64': 'double', 'f32': 'float'}
PATHS = {
    'fused': ({}, None, lambda t, it: {
        'riccati': f'mpcb::row_riccati_kernel<{it}, false>', 'forward': f'mpcb::fwd_rm_kernel<double, {it}>'}),
    'two': ({'MPCB_FUSE_P12': '0'}, None, lambda t, it: {
        'nominal': f'mpcb::nominal_row_kernel<double, {it}, false, true>',
        'riccati': f'mpcb::riccati_kernel_f64<true, {it}, true>', 'forward': f'mpcb::fwd_rm_kernel<double, {it}>'}),
    'notan': ({'MPCB_P1_TAN': '0'}, None, lambda t, it: {
        'nominal': f'mpcb::nominal_row_kernel<double, {it}, false, false>',
        'riccati': f'mpcb::riccati_kernel_f64<true, {it}, false>', 'forward': f'mpcb::fwd_rm_kernel<double, {it}>'}),
    'row32': ({}, None, lambda t, it: {
        'nominal': f'mpcb::nominal_row_kernel<float, {it}, false, false>',
        'riccati': f'mpcb::riccati_kernel_f32<true, {it}, false>', 'forward': f'mpcb::fwd_rm_kernel<float, {it}>'}),
    'small': ({'MPCB_SMALL_MAX': '1000000'}, None, lambda t, it: {
        'nominal': f'mpcb::nominal_row_kernel<{T[t]}, {it}, false, false>',
        'riccati': f'mpcb::box_kernel_{t}<0>', 'linearise': f'mpcb::lin_kernel<{T[t]}>'}),
    'single': ({'MPCB_SPLIT_MIN_BATCH': str(1 << 40)}, None, lambda t, it: {
        'riccati': f'mpcb::solve_kernel<{T[t]}, 0>'}),
    'thread': ({}, 16385, lambda t, it: {
        'nominal': f'mpcb::nominal_kernel<{T[t]}, {it}>',
        'riccati': f'mpcb::riccati_kernel_{t}<{"true" if t == "f64" else "false"}, {it}, false>',
        'forward': f'mpcb::forward_kernel<{T[t]}, false, {it}>'}),
    'lanequad': ({}, None, lambda t, it: {
        'nominal': f'mpcb::nominal_quad_kernel<{T[t]}, {it}>',
        'riccati': f'mpcb::riccati_kernel_{t}<true, {it}, false>', 'forward': f'mpcb::fwd_rm_kernel<{T[t]}, {it}>'}),
    # input box
    'box': ({}, None, lambda t, it: dict(
        {'riccati': f'mpcb::row_riccati_kernel<{it}, false>'} if t == 'f64' else
        {'nominal': f'mpcb::nominal_row_kernel<float, {it}, false, false>',
         'riccati': f'mpcb::riccati_kernel_f32<true, {it}, false>'},
        forward=f'mpcb::as_kernel_{t}<true, {it}>')),
    'box_ipm': ({}, None, lambda t, it: {
        'riccati': f'mpcb::row_riccati_kernel<{it}, false>', 'forward': f'mpcb::as_kernel_f64<true, {it}>'}),
    'box_v1': ({'MPCB_BOX_IMPL': 'v1'}, None, lambda t, it: {'riccati': 'mpcb::solve_kernel<double, 1>'}),
}


def _use_wind(mode, alt):
    """Wind on half of the cases, so that every path sees it in both modes and both variants."""
    return (mode == 'iterate') != (alt == 'b')


@functools.lru_cache(maxsize=None)
def _inputs(N, B, dtype):
    """make_inputs('c3'), the iterate xref + N(0, 0.05), uref + N(0, 1) and the c5 wind draw of
    the same instances, as the handle of ``dtype`` sees them."""
    ids = np.arange(B, dtype=np.uint64)
    inp = make_inputs('c3', ids=ids, N=N)
    rng = np.random.default_rng(3)
    inp['xbar'] = inp['xref'] + rng.normal(scale=0.05, size=(B, N + 1, 12))
    inp['ubar'] = inp['uref'] + rng.normal(scale=1.0, size=(B, N, 4))
    inp['wind'] = make_wind(draws(1003, ids))
    c = _cast(dtype)
    return {k: c(v) for k, v in inp.items()}


@functools.lru_cache(maxsize=None)
def _oracle(N, B, mode, alt, dtype, boxed, max_as_iter=200, groups=ac.GROUPS):
    """One reference per case, shared by the paths that solve the same problem; never modified."""
    inp = _inputs(N, B, dtype)
    kw = ac.fields(alt=alt, groups=groups, box='input' if boxed else 'none', dtype=dtype)
    spec = OcpSpec(N=N, max_as_iter=max_as_iter, **ac.spec_kwargs(kw))
    wind = inp['wind'] if _use_wind(mode, alt) else None
    it = dict(mode='iterate', xbar=inp['xbar'], ubar=inp['ubar']) if mode == 'iterate' else {}
    o = mpc_solve(inp['x0'], inp['xref'], inp['uref'], spec, wind=wind, return_lin=True, **it)
    return o, spec


def _handle(path, N, B, dtype, monkeypatch, **cfg):
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    env, max_batch, _ = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return BatchedMPC(MPCConfig(N=N, dtype=dtype, **cfg), max_batch=max_batch or B)


def _solve12(m, N, B, mode, alt, dtype):
    inp = _inputs(N, B, dtype)
    wind = inp['wind'] if _use_wind(mode, alt) else None
    if mode == 'iterate':
        m.solve_iterate(inp['x0'], inp['xbar'], inp['ubar'], inp['xref'], inp['uref'], wind=wind)
    else:
        m.solve(inp['x0'], inp['xref'], inp['uref'], wind=wind)
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for t in (m.get_control(), m.get_state_trajectory(),
                                             m.get_input_trajectory(), m.get_status())]


def _kernels_are(m, B, mode, expected):
    k = m.last_kernels()
    assert k == m.plan_kernels(B, iterate=mode == 'iterate')
    assert k == expected


def _noise_move(o, inp, spec, trials=2, rel=2.0 ** -22):
    """The unconstrained reference's own move under fp32-level data noise: [A|B] scaled entrywise
    by (1 + 2^-22 N(0, 1)) (oracle.ocp.fp32_sensitivity's perturbation) through riccati_solve;
    the largest normwise move of u0, X and U over the instances."""
    rs = np.random.default_rng(0)
    worst = 0.0
    for _ in range(trials):
        A = o['A'] * (1.0 + rel * rs.standard_normal(o['A'].shape))
        Bm = o['B'] * (1.0 + rel * rs.standard_normal(o['B'].shape))
        dx, du, _, _ = riccati_solve(A, Bm, o['gap'], inp['x0'] - o['xbar'][:, 0], o['xbar'], o['ubar'],
                                     inp['xref'], inp['uref'], spec)
        X, U = o['xbar'] + dx, o['ubar'] + du
        worst = max(worst, relerr(U[:, 0], o['u0']).max(), relerr(X, o['X']).max(), relerr(U, o['U']).max())
    return worst


def _accept_free(tag, o, u0, X, U, st, dtype, tol=None):
    """The acceptance of an unconstrained 12/4 solve against its oracle ``o`` (shared with
    tests/test_gpu_abi.py, which holds its baselines to the bounds of this file)."""
    e = [relerr(u0, o['u0']).max(), relerr(X, o['X']).max(), relerr(U, o['U']).max()]
    if tol is None:
        tol = 1e-9 if dtype == 'f64' else 5e-5
    print(f'{tag}: max rel err u0 {e[0]:.2e} X {e[1]:.2e} U {e[2]:.2e} (bound {tol:.1e})')
    assert (st == o['status']).all() and (st == 0).all()
    assert max(e) < tol


def _check_free(path, N, B, mode, alt, dtype, monkeypatch, tol=None):
    o, spec = _oracle(N, B, mode, alt, dtype, False)
    m = _handle(path, N, B, dtype, monkeypatch, **ac.fields(alt=alt, box='none', dtype=dtype))
    u0, X, U, st = _solve12(m, N, B, mode, alt, dtype)
    _kernels_are(m, B, mode, PATHS[path][2](dtype, _it(mode)))
    _accept_free(f'ALT-{alt} {path} {dtype} N={N} {mode}', o, u0, X, U, st, dtype, tol)


@pytest.mark.parametrize('alt', ALTS)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('N', [1, 2, 6])
@pytest.mark.parametrize('path,dtype', [
    ('fused', 'f64'), ('two', 'f64'), ('notan', 'f64'), ('row32', 'f32'), ('small', 'f64'), ('small', 'f32'),
    ('single', 'f64'), ('single', 'f32')])
def test_unconstrained_path_matches_oracle(path, dtype, N, mode, alt, monkeypatch):
    """fused rollout + Riccati with the 16-lane forward pass; the same as two launches; the
    captured-scalar P2; the fp32 row rollout + matrix-core Riccati; the small-chunk cached [A|B]
    passes; the single-kernel solver."""
    _check_free(path, N, B12, mode, alt, dtype, monkeypatch)


@pytest.mark.parametrize('alt', ALTS)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_thread_per_instance_path_matches_oracle(dtype, mode, alt, monkeypatch):
    """A handle above the 16384-instance small-chunk threshold (thread-per-instance rollout and
    forward pass) solving B = 37 instances at N = 6."""
    _check_free('thread', 6, B12, mode, alt, dtype, monkeypatch)


@pytest.mark.parametrize('alt', ALTS)
@pytest.mark.parametrize('mode', MODES)
def test_lane_quad_rollout_matches_oracle_fp64(mode, alt, monkeypatch):
    """N = 130: the row rollout's LDS carve exceeds 64 KiB in fp64, so the lane-quad rollout runs."""
    _check_free('lanequad', 130, 5, mode, alt, 'f64', monkeypatch)


@pytest.mark.parametrize('alt', ALTS)
def test_lane_quad_rollout_matches_oracle_fp32_iterate(alt, monkeypatch):
    """N = 260, fp32 (the lane-quad rollout's fp32 threshold), iterate mode.  No measured precedent
    for an fp32 horizon this long, so the bound is max(5e-5, 10 x the reference's own move under
    fp32-level noise on [A|B]) (_noise_move: two draws of 2-ulp noise understate the rounding
    accumulated over N stages, hence the factor 10).  Measured: move 2.0e-6 (ALT-a) and 1.2e-6
    (ALT-b), so the bound is 5e-5 in both variants."""
    N, B = 260, 5
    o, spec = _oracle(N, B, 'iterate', alt, 'f32', False)
    move = _noise_move(o, _inputs(N, B, 'f32'), spec)
    tol = max(5e-5, 10.0 * move)
    print(f'ALT-{alt} N={N} f32: reference move under fp32 noise {move:.2e} -> bound {tol:.2e}')
    _check_free('lanequad', N, B, 'iterate', alt, 'f32', monkeypatch, tol=tol)


# ------------------------------------------------------------------------------ 12/4 input box
def _on_bound(U, lbu, ubu):
    return (np.abs(U - lbu) <= ON_BOUND) | (np.abs(U - ubu) <= ON_BOUND)


def _check_box(path, N, B, mode, alt, dtype, monkeypatch, max_as_iter=200, groups=ac.GROUPS):
    from test_gpu_fuzz import qp_objective
    o, spec = _oracle(N, B, mode, alt, dtype, True, max_as_iter, groups)
    inp = _inputs(N, B, dtype)
    # conditions on the oracle's output that keep the case from passing vacuously
    frac = _on_bound(o['U'], spec.lbu, spec.ubu).mean()
    nfb = int(o['fallback'].sum())
    print(f'ALT-{alt} {path} {dtype} N={N} {mode}: oracle has {100 * frac:.0f} % of U on a bound, '
          f'{nfb} instances through the interior point')
    if alt == 'a' and N == 6 and B == B12 and groups == ac.GROUPS:
        assert frac >= 0.10
        assert nfb >= 1
    kw = ac.fields(alt=alt, groups=groups, box='input', dtype=dtype)
    m = _handle(path, N, B, dtype, monkeypatch, max_as_iter=max_as_iter, **kw)
    u0, X, U, st = _solve12(m, N, B, mode, alt, dtype)
    expected = PATHS[path][2](dtype, _it(mode))
    if 'model' not in groups and 'riccati' in expected:   # the default diagonal inertia's instantiation
        expected['riccati'] = expected['riccati'].replace(', false>', ', true>')
    _kernels_are(m, B, mode, expected)
    _accept_box(f'ALT-{alt} {path} {dtype} N={N} {mode}', o, spec, inp, u0, X, U, st, dtype)


def _accept_box(tag, o, spec, inp, u0, X, U, st, dtype):
    """The acceptance of a 12/4 input-box solve against its oracle ``o`` (shared with
    tests/test_gpu_abi.py)."""
    from test_gpu_fuzz import qp_objective
    B = u0.shape[0]
    eu, ex, eU = relerr(u0, o['u0']), relerr(X, o['X']), relerr(U, o['U'])
    print(f'{tag}: max rel err u0 {eu.max():.2e} X {ex.max():.2e} U {eU.max():.2e}')
    assert (st == o['status']).all() and (st == 0).all()
    tb = 1e-6 if dtype == 'f64' else 2e-4
    assert (U >= spec.lbu - tb).all() and (U <= spec.ubu + tb).all()
    if dtype == 'f64':
        assert max(eu.max(), ex.max(), eU.max()) < 1e-9
        return
    x0, xref, uref = inp['x0'], inp['xref'], inp['uref']
    sens = fp32_sensitivity(o, x0, xref, uref, spec)
    ill = sens > 1e-5
    gap = qp_objective(o, U, x0, xref, uref, spec) / np.abs(qp_objective(o, o['U'], x0, xref, uref, spec)) - 1.0
    over = ~ill & ((eu >= 5e-5) | (ex >= 5e-5) | (eU >= 5e-5))
    print(f'  fp32 box: {int(ill.sum())} of {B} instances fp32-ill-conditioned (sensitivity max {sens.max():.1e}); '
          f'{int(over.sum())} others beyond the bound; objective gap max {gap.max():.2e}')
    assert ill.sum() <= 0.05 * B
    assert not over.any()
    assert (gap < 1e-5).all()


@pytest.mark.parametrize('alt', ALTS)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('N', [2, 6])
@pytest.mark.parametrize('path,dtype', [('box', 'f64'), ('box', 'f32'), ('box_ipm', 'f64'), ('box_v1', 'f64')])
def test_input_box_path_matches_oracle(path, dtype, N, mode, alt, monkeypatch):
    """The active set with its interior-point hand-over (fp64), the same plus the fp64-residual
    refinement (fp32), the box solved by the interior point (max_as_iter = 1: every instance the
    first pass leaves unconverged is handed over), and the single-kernel box solver
    (MPCB_BOX_IMPL=v1), on ALT's per-channel box."""
    _check_box(path, N, B12, mode, alt, dtype, monkeypatch, max_as_iter=1 if path == 'box_ipm' else 200)


# ------------------------------------------------------------------------------ localisation
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('path,group', [('fused', 'weights'), ('fused', 'model'), ('fused', 'time'),
                                        ('box', 'weights'), ('box', 'model'), ('box', 'time'), ('box', 'box')])
def test_one_group_swapped_to_alt(path, group, mode, monkeypatch):
    """The default config with ONE group of fields swapped to ALT (weights; model constants; ALT-b's
    dt and cost_scale; the box), on the default fp64 path and the fp64 box path at N = 2, B = 5: a
    failure in the path matrix above then points at a table."""
    N, B, groups = 2, 5, (group,)
    if path == 'box':
        _check_box('box', N, B, mode, 'b', 'f64', monkeypatch, groups=groups)
        return
    o, _ = _oracle(N, B, mode, 'b', 'f64', False, 200, groups)
    m = _handle('fused', N, B, 'f64', monkeypatch, **ac.fields(alt='b', groups=groups, box='none'))
    u0, X, U, st = _solve12(m, N, B, mode, 'b', 'f64')
    dj = 'false' if group == 'model' else 'true'
    _kernels_are(m, B, mode, {'riccati': f'mpcb::row_riccati_kernel<{_it(mode)}, {dj}>',
                              'forward': f'mpcb::fwd_rm_kernel<double, {_it(mode)}>'})
    e = [relerr(u0, o['u0']).max(), relerr(X, o['X']).max(), relerr(U, o['U']).max()]
    print(f'only {group} {mode}: max rel err u0 {e[0]:.2e} X {e[1]:.2e} U {e[2]:.2e}')
    assert (st == o['status']).all() and (st == 0).all()
    assert max(e) < 1e-9


# ------------------------------------------------------------------------------ other entry points
def _moved(fn, args, trials=4):
    """The fp32 bound of each output of the fp64 reference ``fn(*args)``: 8 x its largest move
    under a relative 2^-22 perturbation of the array arguments (the rule of tests/test_gpu_eval.py:
    the perturbation models the rounding of the data only, hence the factor), plus 16 x 2^-24 x
    the output's largest entry.  The second term is the arithmetic's own rounding, which the first
    cannot see on an output that hardly depends on the data (B is mostly model constants times h):
    an entry is accumulated over the four RK4 stages from a handful of fp32 products and sums,
    about 16 operations, each rounding by at most 2^-24 of the largest entry."""
    ref = fn(*args)
    rng = np.random.default_rng(0)
    allow = [0.0] * len(ref)
    for _ in range(trials):
        out = fn(*[a * (1.0 + 2.0 ** -22 * rng.standard_normal(a.shape)) for a in args])
        allow = [max(w, 8.0 * np.abs(a - b).max()) for w, a, b in zip(allow, out, ref)]
    return ref, [w + 16.0 * 2.0 ** -24 * np.abs(r).max() for w, r in zip(allow, ref)]


def _spec_b(dtype, N, full=False, box='none'):
    kw = ac.fields(full=full, alt='b', box=box, dtype=dtype)
    return kw, (FullSpec if full else OcpSpec)(N=N, **ac.spec_kwargs(kw))


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_linearize_and_sim_step_under_alt(dtype):
    """mpcb_linearize against rk4_sens and mpcb_sim_step (T equal to neither dt nor 1/30) against
    rk4_step under ALT-b with wind: fp64 within 1e-12 (the bound of tests/test_gpu_parity.py);
    fp32 within the fp64 reference's move under 2^-22 data noise plus the arithmetic's own rounding
    (_moved)."""
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    N, B, c = 5, 37, _cast(dtype)
    kw, spec = _spec_b(dtype, N)
    m = BatchedMPC(MPCConfig(N=N, dtype=dtype, **kw), max_batch=B)
    rng = np.random.default_rng(5)
    xb, ub = c(rng.uniform(-0.6, 0.6, (B, N + 1, 12))), c(rng.uniform(5.0, 40.0, (B, N, 4)))
    w = c(make_wind(draws(1003, np.arange(B, dtype=np.uint64))))
    got = [t.cpu().numpy().astype(np.float64) for t in m.linearize(xb, ub, wind=w)]   # A, B, x_next

    def lin(xb, ub, w):
        r = [rk4_sens(xb[:, k], ub[:, k], spec.dt, spec.params, w) for k in range(N)]
        return [np.stack([s[i] for s in r], axis=1) for i in (1, 2, 0)]

    Tstep = float(np.float32(0.013)) if dtype == 'f32' else 0.013
    xs = m.sim_step(xb[:, 0], ub[:, 0], T=Tstep, wind=w).cpu().numpy().astype(np.float64)

    def sim(x, u, w):
        return [rk4_step(x, u, Tstep, spec.params, w)]

    if dtype == 'f64':
        ref, allow = lin(xb, ub, w) + sim(xb[:, 0], ub[:, 0], w), [1e-12] * 4
    else:
        (ref, allow), (ref2, allow2) = _moved(lin, (xb, ub, w)), _moved(sim, (xb[:, 0], ub[:, 0], w))
        ref, allow = ref + ref2, allow + allow2
    err = [np.abs(a - b).max() for a, b in zip(got + [xs], ref)]
    print(f'ALT-b {dtype}: ' + '  '.join(f'{n} err {e:.2e} allow {a:.2e}' for n, e, a in zip(('A', 'B', 'x_next', 'sim_step'), err, allow)))
    for e, a in zip(err, allow):
        assert e <= a


def _eval_case(spec, x0, uref, w, p=None, seed=7):
    rng = np.random.default_rng(seed)
    U = uref + rng.standard_normal(uref.shape)
    X = rollout_any(x0, U, spec, w, p) + 0.02 * rng.standard_normal((x0.shape[0], spec.N + 1, x0.shape[1]))
    return X, U


def _eval_metric(a, ref):
    return dict(cost=np.abs(a['cost'] - ref['cost']) / np.maximum(1.0, np.abs(ref['cost'])),
                res_eq=np.abs(a['res_eq'] - ref['res_eq']), res_ineq=np.abs(a['res_ineq'] - ref['res_ineq']),
                res_stat=np.abs(a['res_stat'] - ref['res_stat']) / np.maximum(1.0, ref['res_stat']))


def _check_eval(m, spec, dtype, x0, X, U, xref, uref, w, p, tag):
    """fp64: the bounds of tests/test_gpu_eval.py (_check64); fp32: its rule (_check32: 8 x the
    fp64 reference's move under 2^-22 noise on x0, X, U and the references), here with wind."""
    import test_gpu_eval as ge
    got = ge._np(m.evaluate(X, U, xref, uref, x0=x0, wind=w))
    ref = eval_ref(X, U, xref, uref, spec, x0=x0, wind=w, p25=p)
    assert ref['res_eq'].min() > 1e-3 and ref['res_stat'].min() > 1e-3   # not zeros
    if dtype == 'f64':
        ge._check64(got, ref, spec.N, tag)
        return
    rng = np.random.default_rng(0)
    allow = {k: 0.0 for k in ge.KEYS}
    for _ in range(4):
        q = [a * (1.0 + 2.0 ** -22 * rng.standard_normal(a.shape)) for a in (x0, X, U, xref, uref)]
        mv = _eval_metric(eval_ref(q[1], q[2], q[3], q[4], spec, x0=q[0], wind=w, p25=p), ref)
        allow = {k: max(allow[k], 8.0 * mv[k].max()) for k in ge.KEYS}
    err = {k: v.max() for k, v in _eval_metric(got, ref).items()}
    print(f'{tag} fp32: ' + '  '.join(f'{k} err {err[k]:.2e} allow {allow[k]:.2e}' for k in ge.KEYS))
    for k in ge.KEYS:
        assert err[k] <= allow[k], (tag, k, err[k], allow[k])


@pytest.mark.parametrize('boxed', [False, True])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_evaluate_under_alt(dtype, boxed):
    """mpcb_eval under ALT-b with wind, with and without ALT's box (about half of the hover-centred
    inputs lie above ubu[2] = 22, so res_ineq and the projected gradient are exercised)."""
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    N, B = 6, 7
    kw, spec = _spec_b(dtype, N, box='input' if boxed else 'none')
    inp = _inputs(N, B, dtype)
    c = _cast(dtype)
    X, U = (c(a) for a in _eval_case(spec, inp['x0'], inp['uref'], inp['wind']))
    m = BatchedMPC(MPCConfig(N=N, dtype=dtype, **kw), max_batch=B)
    _check_eval(m, spec, dtype, inp['x0'], X, U, inp['xref'], inp['uref'], inp['wind'], None,
                f'12/4 ALT-b {"box" if boxed else "free"}')


# ------------------------------------------------------------------------------ 17/6
B17 = 13
RIC17 = {('none', 'f64'): 'mpcb::q17::riccati17q_kernel<double, false, false>',
         ('none', 'f32'): 'mpcb::q17::riccati17q_kernel<float, false, false>',
         ('input', 'f64'): 'mpcb::q17::riccati17q_kernel<double, true, true>',
         ('input', 'f32'): 'mpcb::q17::riccati17q_kernel<float, true, false>',
         ('all', 'f64'): 'mpcb::q17::riccati17q_kernel<double, true, false>'}


@functools.lru_cache(maxsize=None)
def _inputs17(N, dtype):
    """The generator of tests/test_gpu_fuzz17.py with stage-varying parameters, T_blast = 4."""
    from test_gpu_fuzz17 import inputs
    rng = np.random.default_rng(17)
    x0, xref, uref, p = inputs(B17, N, rng, True)
    p[..., 24] = 4.0
    xb = x0[:, None, :] + rng.normal(0, 0.03, (B17, N + 1, 17))
    ub = uref + rng.normal(0, 0.5, (B17, N, 6))
    return tuple(_cast(dtype)(a) for a in (x0, xref, uref, p, xb, ub))


@functools.lru_cache(maxsize=None)
def _oracle17(N, mode, alt, dtype, bounds):
    x0, xref, uref, p, xb, ub = _inputs17(N, dtype)
    spec = FullSpec(N=N, **ac.spec_kwargs(ac.fields(full=True, alt=alt, box=bounds, dtype=dtype)))
    it = dict(mode='iterate', xbar=xb, ubar=ub) if mode == 'iterate' else {}
    return mpc_solve17(x0, xref, uref, spec, p, **it), spec


@pytest.mark.parametrize('alt', ALTS)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('bounds,dtype,N', [
    ('none', 'f64', 2), ('none', 'f64', 7), ('input', 'f64', 2), ('input', 'f64', 7), ('all', 'f64', 1),
    ('all', 'f64', 2), ('all', 'f64', 7), ('none', 'f32', 2), ('none', 'f32', 7), ('input', 'f32', 2),
    ('input', 'f32', 7)])
def test_full17_matches_oracle(bounds, dtype, N, mode, alt):
    """The 17/6 model under its own ALT (dense weights of default_rng(11), the 12/4 ALT's model
    constants and dt / cost_scale variants, a per-channel input box, the state box
    1.1 SB_LO - 0.01 .. 0.9 SB_HI + 0.02), acceptance as tests/test_gpu_fuzz17.py with no
    OK-against-MINSTEP allowance.  N = 1 with the state box has no constrained stage: the
    library's empty stage range against the oracle's input-box solve."""
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    from test_gpu_fuzz17 import qp_objective
    x0, xref, uref, p, xb, ub = _inputs17(N, dtype)
    o, spec = _oracle17(N, mode, alt, dtype, bounds)
    assert (o['status'] == 0).all()
    if bounds != 'none':
        frac = _on_bound(o['U'], spec.lbu, spec.ubu).mean()
        print(f'17/6 ALT-{alt} {bounds} {dtype} N={N} {mode}: oracle has {100 * frac:.0f} % of U on a bound')
        assert frac >= 0.20
    m = BatchedMPC(MPCConfig.full(N=N, dtype=dtype, **ac.fields(full=True, alt=alt, box=bounds, dtype=dtype)),
                   max_batch=B17)
    m.set_params(p)
    if mode == 'iterate':
        m.solve_iterate(x0, xb, ub, xref, uref)
    else:
        m.solve(x0, xref, uref)
    torch.cuda.synchronize()
    k = m.last_kernels()
    assert k == m.plan_kernels(B17, iterate=mode == 'iterate')
    assert k == {'nominal': f'mpcb::nominal17q_kernel<{T[dtype]}>', 'riccati': RIC17[bounds, dtype],
                 'linearise': f'mpcb::lin17ws_kernel<{T[dtype]}>'}
    u0, X, U, st = (t.cpu().numpy() for t in (m.get_control(), m.get_state_trajectory(),
                                               m.get_input_trajectory(), m.get_status()))
    _accept17(f'17/6 ALT-{alt} {bounds} {dtype} N={N} {mode}', o, spec, x0, xref, uref, u0, X, U, st, bounds, dtype)


def _accept17(tag, o, spec, x0, xref, uref, u0, X, U, st, bounds, dtype):
    """The acceptance of a 17/6 solve against its oracle ``o`` (shared with tests/test_gpu_abi.py)."""
    from test_gpu_fuzz17 import qp_objective
    N = spec.N
    e = [relerr(u0, o['u0']).max(), relerr(X, o['X']).max(), relerr(U, o['U']).max()]
    print(f'{tag}: rel err u0 {e[0]:.2e} X {e[1]:.2e} U {e[2]:.2e}, '
          f'status {np.bincount(st, minlength=5).tolist()}')
    assert (st == o['status']).all()
    if bounds == 'none':
        if dtype == 'f64':
            assert max(e) <= 1e-9
        else:
            assert e[0] <= 5e-3
        return
    # (N = 1: no state rows, and the objective helper's row maximum needs at least one)
    qspec = spec if (bounds != 'all' or N > 1) else FullSpec(**dict(spec.__dict__, lbx=None, ubx=None))
    Jd, vd = qp_objective(o, U, x0, xref, uref, qspec)
    Jo, _ = qp_objective(o, o['U'], x0, xref, uref, qspec)
    jgap = Jd / np.abs(Jo) - 1.0
    print(f'  objective gap max {jgap.max():.2e}, state-box violation {vd.max():.1e}')
    if dtype == 'f64':
        assert jgap.max() <= 1e-9 and vd.max() <= 1e-9 and max(e) <= 1e-5
    else:
        assert jgap.max() <= 1e-5


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_full17_entry_points_under_alt(dtype):
    """linearize / sim_step / evaluate of the 17/6 model under ALT-b with stage-varying parameters:
    fp64 linearize and sim_step within 1e-11 (the bound of tests/test_gpu_full17.py), fp32 by
    _moved; evaluate with the input box as tests/test_gpu_eval.py."""
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    N = 7
    x0, xref, uref, p, xb, ub = _inputs17(N, dtype)
    kw, spec = _spec_b(dtype, N, full=True, box='input')
    m = BatchedMPC(MPCConfig.full(N=N, dtype=dtype, **kw), max_batch=B17)
    m.set_params(p)
    got = [t.cpu().numpy().astype(np.float64) for t in m.linearize(xb, ub)]

    def lin(xb, ub):
        r = [rk4_sens17(xb[:, k], ub[:, k], p[:, k], spec.dt, spec.params) for k in range(N)]
        return [np.stack([s[i] for s in r], axis=1) for i in (1, 2, 0)]

    Tstep = float(np.float32(0.013)) if dtype == 'f32' else 0.013
    xs = m.sim_step(xb[:, 0], ub[:, 0], T=Tstep).cpu().numpy().astype(np.float64)

    def sim(x, u):
        return [rk4_step17(x, u, p[:, 0], Tstep, spec.params)]

    if dtype == 'f64':
        ref, allow = lin(xb, ub) + sim(xb[:, 0], ub[:, 0]), [1e-11] * 4
    else:
        (ref, allow), (ref2, allow2) = _moved(lin, (xb, ub)), _moved(sim, (xb[:, 0], ub[:, 0]))
        ref, allow = ref + ref2, allow + allow2
    err = [np.abs(a - b).max() for a, b in zip(got + [xs], ref)]
    print(f'17/6 ALT-b {dtype}: ' + '  '.join(f'{n} err {e:.2e} allow {a:.2e}' for n, e, a in zip(('A', 'B', 'x_next', 'sim_step'), err, allow)))
    for e, a in zip(err, allow):
        assert e <= a
    c = _cast(dtype)
    X, U = (c(a) for a in _eval_case(spec, x0, uref, None, p, seed=11))
    _check_eval(m, spec, dtype, x0, X, U, xref, uref, None, p, '17/6 ALT-b box_u')
