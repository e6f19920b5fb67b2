"""mpcb_solve_gains on the GPU (the feedback gains K_k and the cost-to-go Hessian P_0 of one
solve_iterate step, both models) against tests/gains_ref.py: the device is compared with the NumPy
reference, never with itself.  tests/test_gains_ref_cpu.py ties that reference to finite
differences of the oracle's solves.

Metric: per instance and per output |dev - ref|_inf / max(|ref|_inf, 1).  Bounds: fp64 1e-9 (the
project's bound for the vector-Jacobian products); fp32 5e-5 on 12/4 and 5e-4 on 17/6 (the
products' own), the reference reading the data and weights as the fp32 handle holds them.  Each test
prints its measured maxima (DESIGN.md records them).

Shapes are the smallest that reach each code path: one stage and three padding groups (1,1); a
ragged wave (B = 7, 5); the second and third round of the stage-parallel nominal pass over its 16
lanes (N = 17, 33); more waves than workspace slots (37 on 3); on 17/6 more stages than lanes (17),
the reference horizon (60) and two chunks (64 + 6).
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_call as abi   # noqa: E402
import alt_config as ac   # noqa: E402
import vjp17_ref as vr   # noqa: E402
from gains_ref import gains17_ref, gains_ref, relerr   # noqa: E402
from vjp_ref import active_set, vjp_case   # noqa: E402

from oracle.full import FullSpec   # noqa: E402
from oracle.ocp import OcpSpec   # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

KEYS = ('K', 'P0')
BOUND = {('f64', 12): 1e-9, ('f64', 17): 1e-9, ('f32', 12): 5e-5, ('f32', 17): 5e-4}
LB, UB = np.full(4, 5.0), np.full(4, 40.0)
SHAPES12 = [(1, 1), (7, 3), (5, 17), (5, 33)]
SHAPES17 = [(1, 1), (5, 3), (7, 17), (3, 60)]


def _f32(a):
    return None if a is None else np.asarray(a, dtype=np.float32).astype(np.float64)


def _mpc(N, B, dtype='f64', full=False, **kw):
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    return BatchedMPC((MPCConfig.full if full else MPCConfig)(N=N, dtype=dtype, **kw), max_batch=B)


def _spec32(spec):
    spec.Q, spec.R, spec.QN, spec.cost_scale = _f32(spec.Q), _f32(spec.R), _f32(spec.QN), float(np.float32(spec.s))
    if spec.lbu is not None:
        spec.lbu, spec.ubu = _f32(spec.lbu), _f32(spec.ubu)
    return spec


@functools.lru_cache(maxsize=None)
def _case12(B, N, wind=False):
    c = vjp_case(B, N, OcpSpec(N=N), 'hover', wind)
    for v in c.values():
        if v is not None:
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _case17(B, N):
    c = vr.vjp17_case(B, N)
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _mask(B, N, nu):
    m = np.random.default_rng(5).random((B, N, nu)) < 0.5
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _ref12(B, N, masked, wind=False):
    c = _case12(B, N, wind)
    return gains_ref(c['xbar'], c['ubar'], _mask(B, N, 4) if masked else None, OcpSpec(N=N), c['wind'])


@functools.lru_cache(maxsize=None)
def _ref17(B, N, masked):
    c = _case17(B, N)
    return gains17_ref(c['xbar'], c['ubar'], c['p'], _mask(B, N, 6) if masked else None, FullSpec(N=N))


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def _check(got, ref, dtype, nx, tag, keys=KEYS):
    assert np.all(got['status'] == 0), (tag, got['status'])
    bound = BOUND[(dtype, nx)]
    err = {k: relerr(got[k], ref[k]).max() for k in keys}
    print(f'{tag}: ' + '  '.join(f'{k} {err[k]:.2e}/{bound:.0e} (|ref| {np.abs(ref[k]).max():.3g})' for k in keys))
    for k in keys:
        assert err[k] <= bound, (tag, k, err[k])
    return err


def _zero_bits(a):
    """Every entry is +0: no bit set."""
    a = np.ascontiguousarray(a)
    return not a.view({4: np.uint32, 8: np.uint64}[a.itemsize]).any()


def _properties(got, fixed, tag):
    """Clamped rows of K are bitwise 0, P0 is bitwise symmetric."""
    if fixed is not None and np.asarray(fixed).any():
        assert _zero_bits(got['K'][np.asarray(fixed).astype(bool)]), tag
    assert np.array_equal(got['P0'], np.swapaxes(got['P0'], 1, 2)), tag
    assert np.isfinite(got['K']).all() and np.isfinite(got['P0']).all(), tag


def _same(a, b, keys=KEYS + ('status',)):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


def _run12(m, c, **kw):
    return _np(m.solve_iterate_gains(c['xbar'], c['ubar'], wind=c.get('wind'), **kw))


def _run17(m, c, fixed=None, **kw):
    return _np(m.solve_iterate_gains(c['xbar'], c['ubar'], fixed=fixed, **kw))


# ------------------------------------------------------------------------------ 12/4, fp64
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('B,N,wind', [(1, 1, False), (7, 3, True), (5, 17, False), (5, 33, False)])
def test_gains_fp64_matches_reference(B, N, wind, masked):
    c = _case12(B, N, wind)
    fixed = _mask(B, N, 4) if masked else None
    m = _mpc(N, B)   # (a mask is accepted without the box)
    got = _run12(m, c, fixed=fixed)
    _check(got, _ref12(B, N, masked, wind), 'f64', 12, f'12/4 fp64 B={B} N={N} wind={wind} masked={masked}')
    _properties(got, fixed, 'fp64')
    if masked and N > 1:
        assert 0.3 < fixed.mean() < 0.7
    _same(got, _run12(m, c, fixed=fixed))                                # two calls are bit-identical
    k_only, p_only = _run12(m, c, fixed=fixed, want_P0=False), _run12(m, c, fixed=fixed, want_K=False)
    assert 'P0' not in k_only and 'K' not in p_only
    _same(got, k_only, ('K', 'status'))                                  # one output: the bits of both
    _same(got, p_only, ('P0', 'status'))


def test_gains_strides_over_its_slots(monkeypatch):
    """More waves than workspace slots: the kernel's stride loop reuses a slot."""
    B, N = 37, 3
    c = _case12(B, N)
    monkeypatch.setenv('MPCB_GAINS_SLOTS', '3')
    m = _mpc(N, B)
    got = _run12(m, c, fixed=_mask(B, N, 4))
    _check(got, _ref12(B, N, True), 'f64', 12, '12/4 fp64 B=37 N=3, 3 slots')
    _properties(got, _mask(B, N, 4), 'slots')


def test_every_bit_of_the_mask_word_and_the_refusal_beyond_it():
    """The 12/4 kernel keeps one 64-bit mask word per input: N = 64 uses every bit of it, and a mask
    on a longer horizon is refused (the 17/6 kernel reads its mask stage by stage: N = 70 there)."""
    from mpc_blaster_amd import _lib
    B, N = 3, 64
    c = _case12(B, N)
    fixed = _mask(B, N, 4).copy()
    fixed[:, N - 1] = [True, False, True, False]
    fixed[:, 0] = [False, True, False, True]
    got = _run12(_mpc(N, B), c, fixed=fixed)
    _check(got, gains_ref(c['xbar'], c['ubar'], fixed, OcpSpec(N=N)), 'f64', 12, '12/4 fp64 B=3 N=64 masked')
    _properties(got, fixed, 'N=64')
    m = _mpc(65, 2)
    xb, ub = np.zeros((2, 66, 12)), np.zeros((2, 65, 4))
    assert _raw(m, 2, 12, 4, 65, fixed=torch.zeros(2, 65, 4, dtype=torch.uint8, device='cuda')) == -4
    assert b'N <= 64' in m.lib.mpcb_last_error()
    with pytest.raises(_lib.MpcbError, match='-4'):
        m.solve_iterate_gains(xb, ub, fixed=np.zeros((2, 65, 4), dtype=bool))
    assert _raw(m, 2, 12, 4, 65) == 0                                    # without a mask the horizon is free
    B, N = 2, 70
    c17 = _case17(B, N)
    m17 = _mpc(N, B, full=True)
    m17.set_params(c17['p'])
    fx = _mask(B, N, 6)
    _check(_run17(m17, c17, fx), gains17_ref(c17['xbar'], c17['ubar'], c17['p'], fx, FullSpec(N=N)), 'f64', 17,
           '17/6 fp64 B=2 N=70 masked')


def test_fully_clamped_stage_and_empty_mask_in_one_batch():
    B, N = 5, 3
    c = _case12(B, N)
    fixed = _mask(B, N, 4).copy()
    fixed[1, 1] = True      # a stage with all four components clamped
    fixed[2] = False        # an instance with nothing clamped
    m = _mpc(N, B, lbu=LB, ubu=UB)
    got = _run12(m, c, fixed=fixed)
    _check(got, gains_ref(c['xbar'], c['ubar'], fixed, OcpSpec(N=N)), 'f64', 12, '12/4 fully clamped stage / empty mask')
    _properties(got, fixed, 'fully clamped')
    assert _zero_bits(got['K'][1, 1])
    free = _run12(_mpc(N, B), c)
    assert got['K'][2].tobytes() == free['K'][2].tobytes() and got['P0'][2].tobytes() == free['P0'][2].tobytes()


def test_gains_box_end_to_end_set_from_U_and_from_fixed():
    """U from the device's own solve (its clamped components carry the bound itself): the set read
    from U, and the same set given as ``fixed``, bit for bit."""
    B, N = 16, 8
    spec = OcpSpec(N=N, lbu=LB, ubu=UB)
    c = _case12(B, N)
    m = _mpc(N, B, lbu=LB, ubu=UB)
    m.solve_iterate(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'])
    U = m.get_input_trajectory().clone()
    torch.cuda.synchronize()
    assert np.all(m.get_status().cpu().numpy() == 0)
    fixed = active_set(U.cpu().numpy(), spec)
    print(f'end to end: {fixed.any(axis=(1, 2)).sum()} of {B} instances with a clamped component, {fixed.sum()} components')
    assert fixed.any(axis=(1, 2)).sum() >= 8
    ref = gains_ref(c['xbar'], c['ubar'], fixed, spec)
    got = _run12(m, c, U=U)
    assert 'fixed' not in got                                            # the library read the set from U
    _check(got, ref, 'f64', 12, '12/4 fp64 box end to end')
    _properties(got, fixed, 'end to end')
    _same(got, _run12(m, c, fixed=fixed))
    _same(got, _run12(m, c, U=U, active_tol=1e-9))                       # ... and the mask by tolerance
    free = gains_ref(c['xbar'], c['ubar'], None, spec)
    assert (relerr(got['K'], free['K']) > 0.1).sum() >= 8                # the box is not ignored


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_gains_alt_definition(dtype):
    """Dense weights, another model, cost_scale != dt, per-channel bounds, wind (tests/alt_config.py)."""
    B, N = 7, 8
    kw = ac.fields(alt='b', box='input', dtype=dtype)
    spec = OcpSpec(N=N, **ac.spec_kwargs(kw))
    assert spec.s != spec.dt
    cast = _f32 if dtype == 'f32' else (lambda a: a)
    c = {k: cast(v) for k, v in vjp_case(B, N, spec, wind=True).items()}
    rng = np.random.default_rng(3)
    lb, ub = np.asarray(spec.lbu, dtype=np.float64), np.asarray(spec.ubu, dtype=np.float64)
    U = cast(np.clip(c['ubar'] + 30.0 * rng.standard_normal(c['ubar'].shape), lb, ub))
    fixed = active_set(U, spec)
    assert fixed.mean() > 0.2
    ref = gains_ref(c['xbar'], c['ubar'], fixed, spec, c['wind'])
    got = _run12(_mpc(N, B, dtype, **kw), c, U=U)
    _check(got, ref, dtype, 12, f'12/4 ALT-b box wind {dtype}')
    _properties(got, fixed, 'ALT-b')


# ------------------------------------------------------------------------------ 17/6, fp64
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('B,N', SHAPES17)
def test_gains17_fp64_matches_reference(B, N, masked):
    c = _case17(B, N)
    fixed = _mask(B, N, 6) if masked else None
    m = _mpc(N, B, full=True)
    m.set_params(c['p'])
    got = _run17(m, c, fixed)
    _check(got, _ref17(B, N, masked), 'f64', 17, f'17/6 fp64 B={B} N={N} masked={masked}')
    _properties(got, fixed, '17/6 fp64')
    _same(got, _run17(m, c, fixed))
    _same(got, _run17(m, c, fixed, want_P0=False), ('K', 'status'))
    _same(got, _run17(m, c, fixed, want_K=False), ('P0', 'status'))


def test_gains17_fully_clamped_stage_and_empty_mask_in_one_batch():
    B, N = 5, 3
    c = _case17(B, N)
    fixed = _mask(B, N, 6).copy()
    fixed[1, 1] = True
    fixed[2] = False
    m = _mpc(N, B, full=True)
    m.set_params(c['p'])
    got = _run17(m, c, fixed)
    _check(got, gains17_ref(c['xbar'], c['ubar'], c['p'], fixed, FullSpec(N=N)), 'f64', 17,
           '17/6 fully clamped stage / empty mask')
    _properties(got, fixed, '17/6 fully clamped')
    free = _run17(m, c, None)
    assert got['K'][2].tobytes() == free['K'][2].tobytes() and got['P0'][2].tobytes() == free['P0'][2].tobytes()


@pytest.mark.parametrize('kind', ['stage', 'row'])
def test_gains17_parameters_by_stage_and_broadcast(kind):
    B, N = 5, 3
    c = _case17(B, N)
    rng = np.random.default_rng(31)
    if kind == 'stage':
        p = np.repeat(c['p'][:, None, :], N, axis=1)
        p[..., :24] = rng.uniform(-0.5, 0.5, (B, N, 24))
    else:
        p = c['p'][3].copy()
    m = _mpc(N, B, full=True)
    m.set_params(p)
    fixed = _mask(B, N, 6)
    _check(_run17(m, c, fixed), gains17_ref(c['xbar'], c['ubar'], p, fixed, FullSpec(N=N)), 'f64', 17,
           f'17/6 parameters {kind}')


def test_gains17_alt_definition():
    B, N = 5, 3
    kw = ac.fields(full=True, alt='b', groups=('weights', 'model', 'time'), box='none')
    spec = FullSpec(N=N, **ac.spec_kwargs(kw))
    assert spec.s != spec.dt
    c = vr.vjp17_case(B, N, spec)
    fixed = _mask(B, N, 6)
    m = _mpc(N, B, full=True, **kw)
    m.set_params(c['p'])
    got = _run17(m, c, fixed)
    _check(got, gains17_ref(c['xbar'], c['ubar'], c['p'], fixed, spec), 'f64', 17, '17/6 ALT-b')
    _properties(got, fixed, '17/6 ALT-b')


def test_gains17_chunked_run_is_bit_identical(monkeypatch):
    """MPCB_CHUNK = 64 below B = 70: chunks of 64 and 6 instances, the second with a ragged wave."""
    B, N = 70, 3
    c = _case17(B, N)
    fixed = _mask(B, N, 6)
    m = _mpc(N, B, full=True)
    m.set_params(c['p'])
    one = _run17(m, c, fixed)
    monkeypatch.setenv('MPCB_CHUNK', '64')
    mc = _mpc(N, B, full=True)
    mc.set_params(c['p'])
    two = _run17(mc, c, fixed)
    _same(one, two)
    _check(two, _ref17(B, N, True), 'f64', 17, '17/6 chunked 64 + 6')


def test_gains17_mask_from_U_by_tolerance():
    """On 17/6 the Python layer derives the mask from U by solve_iterate_vjp's rule."""
    spec, c = vr.boxed_case()
    B, N = c['ubar'].shape[:2]
    m = _mpc(N, B, full=True, lbu=vr.LBU17, ubu=vr.UBU17)
    m.set_params(c['p'])
    m.solve_iterate(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'])
    U = m.get_input_trajectory().clone()
    assert (m.get_status().cpu().numpy() == 0).all()
    fixed, _ = vr.active_mask(U.cpu().numpy(), spec)
    assert fixed.any(axis=(1, 2)).all()
    got = _run17(m, c, U=U)
    assert np.array_equal(got['fixed'].astype(bool), fixed)
    _check(got, gains17_ref(c['xbar'], c['ubar'], c['p'], fixed, spec), 'f64', 17, '17/6 box end to end')
    _properties(got, fixed, '17/6 end to end')
    mf = _mpc(N, B, 'f32', full=True, lbu=vr.LBU17, ubu=vr.UBU17)
    with pytest.raises(ValueError, match='active_tol'):
        mf.solve_iterate_gains(c['xbar'], c['ubar'], U=U.float())


# ------------------------------------------------------------------------------ agreement with the VJP
def test_K0_rows_are_the_vjp_of_u0_on_the_device():
    """gU = e_m at stage 0 and no gX: mpcb_solve_vjp's gx0 is row m of K_0."""
    B, N = 7, 8
    c = _case12(B, N)
    spec = OcpSpec(N=N, lbu=LB, ubu=UB)
    rng = np.random.default_rng(3)
    U = np.clip(c['ubar'] + 30.0 * rng.standard_normal(c['ubar'].shape), LB, UB)
    m = _mpc(N, B, lbu=LB, ubu=UB)
    K = _run12(m, c, U=U)['K']
    assert active_set(U, spec)[:, 0].any() and not active_set(U, spec)[:, 0].all()
    worst = 0.0
    for i in range(4):
        gU = np.zeros((B, N, 4))
        gU[:, 0, i] = 1.0
        v = _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gU=gU, U=U))
        assert np.all(v['status'] == 0)
        worst = max(worst, relerr(v['gx0'], K[:, 0, i]).max())
    print(f'12/4 K_0 against the VJP of u0: {worst:.2e}')
    assert worst <= 1e-9


def test_K0_rows_are_the_vjp17_of_u0_on_the_device():
    B, N = 5, 3
    c = _case17(B, N)
    fixed = _mask(B, N, 6)
    m = _mpc(N, B, full=True)
    m.set_params(c['p'])
    K = _run17(m, c, fixed)['K']
    worst = 0.0
    for i in range(6):
        gU = np.zeros((B, N, 6))
        gU[:, 0, i] = 1.0
        v = _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gU=gU, fixed=fixed))
        assert np.all(v['status'] == 0)
        worst = max(worst, relerr(v['gx0'], K[:, 0, i]).max())
    print(f'17/6 K_0 against the VJP of u0: {worst:.2e}')
    assert worst <= 1e-9


# ------------------------------------------------------------------------------ status
@pytest.mark.parametrize('where', ['xbar', 'ubar', 'U', 'wind'])
def test_nan_instance_is_isolated(where):
    B, N = 5, 3
    c = dict(_case12(B, N, True))
    U = np.clip(c['ubar'] + 30.0 * np.random.default_rng(3).standard_normal(c['ubar'].shape), LB, UB)
    m = _mpc(N, B, lbu=LB, ubu=UB)
    ok = _run12(m, c, U=U)
    d = {k: (None if v is None else v.copy()) for k, v in c.items()}
    d['U'] = U.copy()
    if where == 'wind':
        d['wind'][1, 2] = np.nan
    else:
        d[where][1, 2, 3] = np.inf if where == 'ubar' else np.nan
    got = _run12(m, d, U=d['U'])
    rest = [0, 2, 3, 4]   # 0, 2 and 3 share the wave of instance 1
    assert got['status'][1] == 1 and np.all(got['status'][rest] == 0)
    for k in KEYS:
        assert np.all(np.isnan(got[k][1])), k
        assert got[k][rest].tobytes() == ok[k][rest].tobytes(), k
    if where == 'U':   # U is not read when the set is given
        _same(ok, _run12(m, c, fixed=active_set(U, OcpSpec(N=N, lbu=LB, ubu=UB))))


@pytest.mark.parametrize('where', ['xbar', 'p'])
def test_gains17_nan_instance_is_isolated(where):
    B, N = 5, 3
    c = _case17(B, N)
    m = _mpc(N, B, full=True)
    m.set_params(c['p'])
    ok = _run17(m, c, _mask(B, N, 6))
    d = {k: c[k].copy() for k in ('xbar', 'ubar', 'p')}
    if where == 'p':
        d['p'][1, 7] = np.nan
    else:
        d[where][1, 2, 3] = np.nan
    m.set_params(d['p'])
    got = _run17(m, d, _mask(B, N, 6))
    rest = [0, 2, 3, 4]
    assert got['status'][1] == 1 and np.all(got['status'][rest] == 0)
    for k in KEYS:
        assert np.all(np.isnan(got[k][1])), k
        assert got[k][rest].tobytes() == ok[k][rest].tobytes(), k


@pytest.mark.parametrize('full', [False, True])
def test_indefinite_masked_hessian_is_qp_fail(full):
    B, N = 5, 3
    nu = 6 if full else 4
    c = _case17(B, N) if full else _case12(B, N)
    R = np.diag([0.05] * 4 + [1e-5] * 2) if full else np.diag([0.05] * 4)
    R[0, 0] = -1e4
    m = _mpc(N, B, full=full, R=R)
    if full:
        m.set_params(c['p'])
    fixed = np.zeros((B, N, nu), dtype=bool)
    fixed[..., 1] = True
    run = (lambda f: _run17(m, c, f)) if full else (lambda f: _run12(m, c, fixed=f))
    assert np.all(run(fixed)['status'] == 4)       # channel 0 is free on every stage
    fixed[..., 0] = True
    assert np.all(run(fixed)['status'] == 0)       # ... and masked out, the rest is positive definite


# ------------------------------------------------------------------------------ the entry point itself
def _raw(m, B, nx, nu, N, U=None, fixed=None, K=True, P0=True, wind_sb=0, Bq=None, dtype=torch.float64):
    """mpcb_solve_gains on zero iterates: the return code."""
    d = lambda *s: torch.zeros(s, dtype=dtype, device='cuda')   # noqa: E731
    xb, ub = d(B + 1, N + 1, nx), d(B + 1, N, nu)
    Kd, Pd = d(B + 1, N, nu, nx), d(B + 1, nx, nx)
    st = torch.zeros(B + 1, dtype=torch.int32, device='cuda')
    P, null = abi._p, ctypes.c_void_p(0)
    rc = m.lib.mpcb_solve_gains(m._h, B if Bq is None else Bq, P(xb), P(ub), P(U), P(fixed), null, wind_sb,
                                P(Kd) if K else null, P(Pd) if P0 else null, P(st), null)
    torch.cuda.synchronize()
    return rc


def test_refusals():
    from mpc_blaster_amd import _lib
    assert 'mpcb_solve_gains' in _lib.EXPORTS and hasattr(_lib.load(), 'mpcb_solve_gains')
    N, B = 3, 2
    m = _mpc(N, B)
    before = m.workspace_bytes
    assert _raw(m, B, 12, 4, N) == 0
    assert m.workspace_bytes == before                                   # the call's workspace is its own
    assert _raw(m, B, 12, 4, N, K=False) == 0 and _raw(m, B, 12, 4, N, P0=False) == 0
    assert _raw(m, B, 12, 4, N, K=False, P0=False) == -1                 # MPCB_E_INVALID: both outputs NULL
    assert _raw(m, B, 12, 4, N, Bq=B + 1) == -1                          # B > max_batch
    assert _raw(m, B, 12, 4, N, wind_sb=-3) == -1                        # a negative stride
    mb = _mpc(N, B, lbu=LB, ubu=UB)
    assert _raw(mb, B, 12, 4, N) == -1 and b'U' in mb.lib.mpcb_last_error()   # the box with neither U nor fixed
    assert _raw(mb, B, 12, 4, N, U=torch.zeros(B, N, 4, dtype=torch.float64, device='cuda')) == 0
    assert _raw(mb, B, 12, 4, N, fixed=torch.zeros(B, N, 4, dtype=torch.uint8, device='cuda')) == 0
    m17 = _mpc(N, B, full=True)
    b17 = m17.workspace_bytes
    assert _raw(m17, B, 17, 6, N) == 0 and m17.workspace_bytes == b17
    assert _raw(m17, B, 17, 6, N, K=False, P0=False) == -1 and _raw(m17, B, 17, 6, N, Bq=B + 1) == -1
    mx = _mpc(N, B, full=True, lbu=vr.LBU17, ubu=vr.UBU17, lbx=ac.SB_LO, ubx=ac.SB_HI)
    assert _raw(mx, B, 17, 6, N) == -4                                   # MPCB_E_UNSUPPORTED: the state box
    with pytest.raises(_lib.MpcbError):
        m17.solve_iterate_gains(np.zeros((B, N + 1, 17)), np.zeros((B, N, 6)), wind=np.zeros((B, 3)))
    with pytest.raises(ValueError):
        m.solve_iterate_gains(np.zeros((B, N + 1, 12)), np.zeros((B, N, 4)), want_K=False, want_P0=False)
    with pytest.raises(ValueError):
        m.solve_iterate_gains(np.zeros((B, N + 1, 12)), np.zeros((B, N, 4)), active_tol=1e-6)
    with pytest.raises(ValueError, match='fixed'):
        m.solve_iterate_gains(np.zeros((B, N + 1, 12)), np.zeros((B, N, 4)), fixed=np.zeros((B, N, 3)))


@pytest.mark.parametrize('full', [False, True])
def test_outputs_at_element_alignment_between_guard_bands(full):
    """K and P0 offset to element-only alignment inside sentinel-filled allocations: the bits of the
    aligned call, nothing written outside the views, a NULL output's array untouched."""
    B, N = 5, 3
    nx, nu = (17, 6) if full else (12, 4)
    c = _case17(B, N) if full else _case12(B, N)
    fixed = _mask(B, N, nu)
    m = _mpc(N, B, full=full)
    if full:
        m.set_params(c['p'])
    ref = _run17(m, c, fixed) if full else _run12(m, c, fixed=fixed)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')   # noqa: E731
    xb, ub = t(c['xbar']), t(c['ubar'])
    fx = torch.tensor(np.ascontiguousarray(fixed), dtype=torch.uint8, device='cuda')
    P, null = abi._p, ctypes.c_void_p(0)
    for wK, wP in ((True, True), (True, False), (False, True)):
        K, P0 = abi.guarded((B, N, nu, nx), torch.float64), abi.guarded((B, nx, nx), torch.float64)
        st = abi.guarded((B,), torch.int32)
        rc = m.lib.mpcb_solve_gains(m._h, B, P(xb), P(ub), null, P(fx), null, 0, P(K) if wK else null,
                                    P(P0) if wP else null, P(st), null)
        torch.cuda.synchronize()
        assert rc == 0
        K.check(), P0.check(), st.check()
        assert (st.view == 0).all()
        if wK:
            assert K.view.cpu().numpy().tobytes() == ref['K'].tobytes()
        else:
            assert K.untouched()
        if wP:
            assert P0.view.cpu().numpy().tobytes() == ref['P0'].tobytes()
        else:
            assert P0.untouched()


# ------------------------------------------------------------------------------ fp32
@pytest.mark.parametrize('masked', [False, True])
def test_gains_fp32(masked):
    B, N = 7, 20
    spec = _spec32(OcpSpec(N=N))
    c = {k: _f32(v) for k, v in _case12(B, N).items()}
    fixed = _mask(B, N, 4) if masked else None
    ref = gains_ref(c['xbar'], c['ubar'], fixed, spec)
    got = _run12(_mpc(N, B, 'f32'), c, fixed=fixed)
    assert got['K'].dtype == np.float32
    _check(got, ref, 'f32', 12, f'12/4 fp32 B={B} N={N} masked={masked}')
    _properties(got, fixed, 'fp32')


@pytest.mark.parametrize('masked', [False, True])
def test_gains17_fp32(masked):
    B, N = 7, 17
    c = {k: _f32(v) for k, v in _case17(B, N).items()}
    spec = FullSpec(N=N)
    spec.Q, spec.R, spec.QN, spec.cost_scale = _f32(spec.Q), _f32(spec.R), _f32(spec.QN), float(np.float32(spec.s))
    fixed = _mask(B, N, 6) if masked else None
    m = _mpc(N, B, 'f32', full=True)
    m.set_params(c['p'])
    ref = gains17_ref(c['xbar'], c['ubar'], c['p'], fixed, spec)
    got = _run17(m, c, fixed)
    _check(got, ref, 'f32', 17, f'17/6 fp32 B={B} N={N} masked={masked}')
    _properties(got, fixed, '17/6 fp32')
