"""mpcb_sim_step_vjp on the GPU (the reverse mode of the plant step), ``sim_step_diff`` and
``closed_loop_diff``, against tests/simvjp_ref.py: the device is compared with the NumPy reference,
which tests/test_simvjp_ref_cpu.py ties to central differences of the oracle.

Metric: tests/test_gpu_vjp.py ``relerr``, per instance and per output.  Bounds: fp64 BOUND['f64'] =
1e-9.  fp32 by the rule of the fp32 cases of tests/test_gpu_pm.py: the reference reads fp32-rounded
inputs, its own move under a seeded +-2^-22 relative perturbation of every input is measured, and the
device is held to max(5e-5, 10 x move), per output.  Shapes: B = 1, 5 and 300 (more than one
256-thread block, the last one partial).  Draw (seed 4, as tests/test_gpu_pm.py): x in
U(-0.5, 0.5), u in U(0, 65), wind in U(-2, 2), gxn ~ N(0, 1), vehicles pm_models.  Each test prints
its measured maxima (DESIGN.md records them).
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_call as ab   # noqa: E402
import simvjp_ref as sr   # noqa: E402
from pm_ref import pack_params, pm_models   # noqa: E402
from test_gpu_vjp import BOUND, _mpc, relerr   # noqa: E402

from oracle.ocp import OcpSpec   # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

KEYS = ('gx', 'gu', 'gwind', 'gmodel')
COLS = dict(gx=12, gu=4, gwind=3, gmodel=14)
TD = {'f64': torch.float64, 'f32': torch.float32}
SHAPES = (1, 5, 300)
BMAX = 300
E_INVALID, E_UNSUPPORTED = -1, -4
SPEC = OcpSpec(N=3)
T = SPEC.dt


def _f32(a):
    return None if a is None else np.asarray(a, dtype=np.float32).astype(np.float64)


def _pert(rng, a):
    return None if a is None else a * (1.0 + 2.0 ** -22 * rng.choice([-1.0, 1.0], size=np.shape(a)))


@functools.lru_cache(maxsize=None)
def _case():
    rng = np.random.default_rng(4)
    c = dict(x=rng.uniform(-0.5, 0.5, (BMAX, 12)), u=rng.uniform(0, 65, (BMAX, 4)), wind=rng.uniform(-2, 2, (BMAX, 3)),
             M=pm_models(BMAX, SPEC), g=rng.standard_normal((BMAX, 12)))
    for a in c.values():
        a.setflags(write=False)
    return c


def _rows(c, B, model='pi', wind='pi'):
    """The first B instances; model / wind: 'pi' per instance, 'bc' the first row broadcast, None."""
    pick = lambda a, how: None if how is None else (a[:B] if how == 'pi' else a[:1])   # noqa: E731
    return dict(x=c['x'][:B], u=c['u'][:B], g=c['g'][:B], M=pick(c['M'], model), wind=pick(c['wind'], wind))


@functools.lru_cache(maxsize=None)
def _ref(dtype, model='pi', wind='pi', own=False):
    """(reference at BMAX instances, fp32: the per-output bound by the rule of the module docstring);
    computed once per variant and shared, instance b's row does not depend on B.  ``own``: the
    record of the spec's own vehicle (what a handle without records flies)."""
    c = _rows(_case(), BMAX, model, wind)
    if own:
        c['M'] = pack_params(SPEC.params)[None]
    if dtype == 'f32':
        c = {k: _f32(v) for k, v in c.items()}
    ref = sr.simvjp_ref(c['x'], c['u'], c['g'], T, SPEC, c['M'], c['wind'])
    bound = {k: BOUND['f64'] for k in KEYS}
    if dtype == 'f32':
        rng = np.random.default_rng(0)
        p = {k: _pert(rng, v) for k, v in c.items()}
        moved = sr.simvjp_ref(p['x'], p['u'], p['g'], T, SPEC, p['M'], p['wind'])
        move = {k: relerr(moved[k], ref[k]).max() for k in KEYS}
        bound = {k: max(BOUND['f32'], 10.0 * move[k]) for k in KEYS}
        print(f'fp32 reference move ({model}, {wind}, own={own}): ' + '  '.join(f'{k} {move[k]:.2e}' for k in KEYS))
    return ref, bound


def _t(a, dtype):
    return None if a is None else torch.as_tensor(np.array(a), dtype=TD[dtype], device='cuda')


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}


def _check(got, ref, bound, B, tag, keys=KEYS):
    err = {k: relerr(got[k], ref[k][:B]).max() for k in keys}
    print(f'{tag}: ' + '  '.join(f'{k} {err[k]:.2e}/{bound[k]:.1e}' for k in keys))
    for k in keys:
        assert got[k].shape == (B, COLS[k]) and err[k] <= bound[k], (tag, k, err[k], bound[k])


def _raw(m, B, a, o, model_sb=None, wind_sb=None, T_=T, stream=0):
    """mpcb_sim_step_vjp with pointers and strides as given; a: x, u, g, wind, M; o: the four outputs
    (missing / None = NULL)."""
    if wind_sb is None:
        wind_sb = 3 if a.get('wind') is not None else 0
    if model_sb is None:
        model_sb = 14 if a.get('M') is not None else 0
    return m.lib.mpcb_sim_step_vjp(m._h, B, ab._p(a['x']), ab._p(a['u']), ab._p(a.get('wind')), wind_sb,
                                   ab._p(a.get('M')), model_sb, float(T_), ab._p(a['g']),
                                   *(ab._p(o.get(k)) for k in KEYS), ab._p(stream))


def _dev_case(B, dtype, **kw):
    return {k: _t(v, dtype) for k, v in _rows(_case(), B, **kw).items()}


def _outs(B, dtype, keys=KEYS):
    return {k: torch.full((B, COLS[k]), 7.0, dtype=TD[dtype], device='cuda') for k in keys}


# ------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('B', SHAPES)
def test_all_outputs_match_reference(dtype, B):
    m = _mpc(3, B, dtype)
    c = _rows(_case(), B)
    # per-instance records and wind
    ref, bound = _ref(dtype)
    got = _np(m.sim_step_vjp(c['x'], c['u'], c['g'], wind=c['wind'], model=c['M'], want=KEYS))
    _check(got, ref, bound, B, f'{dtype} B={B} per-instance')
    # one record and one wind row for all: rows per instance, the reference at the broadcast record
    ref, bound = _ref(dtype, 'bc', 'bc')
    got = _np(m.sim_step_vjp(c['x'], c['u'], c['g'], wind=c['wind'][:1], model=c['M'][:1], want=KEYS))
    _check(got, ref, bound, B, f'{dtype} B={B} broadcast')
    # model_sb = 16 with NaN in the two pad elements
    ref, bound = _ref(dtype)
    Mp = np.concatenate([c['M'], np.full((B, 2), np.nan)], axis=1)
    got = _np(m.sim_step_vjp(c['x'], c['u'], c['g'], wind=c['wind'], model=Mp, want=KEYS))
    assert all(np.isfinite(v).all() for v in got.values())
    _check(got, ref, bound, B, f'{dtype} B={B} model_sb=16')
    # wind = None with gwind requested
    ref, bound = _ref(dtype, 'pi', None)
    got = _np(m.sim_step_vjp(c['x'], c['u'], c['g'], model=c['M'], want=KEYS))
    _check(got, ref, bound, B, f'{dtype} B={B} no wind')
    # model = None: the handle's vehicle, against the reference and against the call given its record
    ref, bound = _ref(dtype, None, 'pi', own=True)
    got = _np(m.sim_step_vjp(c['x'], c['u'], c['g'], wind=c['wind'], want=KEYS))
    _check(got, ref, bound, B, f'{dtype} B={B} handle vehicle')
    rec = _np(m.sim_step_vjp(c['x'], c['u'], c['g'], wind=c['wind'], model=m.pack_model(), want=KEYS))
    _check(got, rec, bound, B, f'{dtype} B={B} handle vehicle against its record', keys=('gx', 'gu', 'gmodel'))


# ------------------------------------------------------------------------------ 2. output selection
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_output_selection_and_reproducibility(dtype):
    B = 300
    m = _mpc(3, B, dtype)
    c = _rows(_case(), B)
    ref, bound = _ref(dtype)
    for model in (c['M'], None):
        if model is None:
            ref, bound = _ref(dtype, None, 'pi', own=True)
        call = lambda want: m.sim_step_vjp(c['x'], c['u'], c['g'], wind=c['wind'], model=model, want=want)   # noqa: E731
        full = call(KEYS)
        for want in [(k,) for k in KEYS] + [('gx', 'gu'), KEYS]:
            out = call(want)
            assert tuple(out) == tuple(want)
            _check(_np(out), ref, bound, B, f'{dtype} records={model is not None} want={want}', keys=want)
        again = call(KEYS)
        torch.cuda.synchronize()
        assert all(ab.same_bits(full[k], again[k]) for k in KEYS)


# ------------------------------------------------------------------------------ 3. the forward kernels
def test_consistent_with_linearize_and_sim_step_unchanged():
    B = 300
    c = _rows(_case(), B)
    m = _mpc(1, B)   # N = 1: linearize gives one [A | B] per instance at (x, u)
    x, u, w = (_t(c[k], 'f64') for k in ('x', 'u', 'wind'))
    xbar = torch.stack([x, x], dim=1).contiguous()
    A, Bm, _ = m.linearize(xbar, u.unsqueeze(1).contiguous(), wind=w)
    g = _t(c['g'], 'f64')
    before = m.sim_step(x, u, wind=w, T=T).clone()
    pm_before = m.sim_step(x, u, wind=w, T=T, model=c['M']).clone()
    got = m.sim_step_vjp(x, u, g, T=m.cfg.dt, wind=w)
    ex = torch.einsum('bij,bi->bj', A[:, 0], g)
    eu = torch.einsum('bij,bi->bj', Bm[:, 0], g)
    e = (relerr(got['gx'].cpu().numpy(), ex.cpu().numpy()).max(), relerr(got['gu'].cpu().numpy(), eu.cpu().numpy()).max())
    print(f'against the device\'s own linearize at N = 1: gx {e[0]:.2e}  gu {e[1]:.2e} / 1e-9')
    assert max(e) <= 1e-9
    m.sim_step_vjp(x, u, g, T=T, wind=w, model=c['M'], want=KEYS)
    assert ab.same_bits(before, m.sim_step(x, u, wind=w, T=T))
    m.sim_step_vjp(x, u, g, T=T, wind=w, want=KEYS)
    assert ab.same_bits(pm_before, m.sim_step(x, u, wind=w, T=T, model=c['M']))


# ------------------------------------------------------------------------------ 4. the NaN rule
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('records', [True, False])
def test_nan_rule(dtype, records):
    B, bad = 300, 257
    m = _mpc(3, B, dtype)
    c = _rows(_case(), B)
    if not records:
        c['M'] = None
    wants = (KEYS, ('gu',), ('gwind', 'gmodel'))
    # (the clean run of the same request: the gx / gu-only kernel is another instantiation)
    clean = {w: m.sim_step_vjp(c['x'], c['u'], c['g'], wind=c['wind'], model=c['M'], want=w) for w in wants}
    # x[0] enters no derivative and gxn[0] only gx[0]: the check sum alone carries those
    for key, col in (('x', 0), ('x', 4), ('u', 2), ('g', 0), ('wind', 1)) + ((('M', 0), ('M', 9)) if records else ()):
        a = {k: (None if v is None else v.copy()) for k, v in c.items()}
        a[key][bad, col] = np.nan
        for want in wants:
            out = m.sim_step_vjp(a['x'], a['u'], a['g'], wind=a['wind'], model=a['M'], want=want)
            torch.cuda.synchronize()
            for k in want:
                assert bool(torch.isnan(out[k][bad]).all()), (key, col, k)
                keep = torch.arange(B, device='cuda') != bad
                assert ab.same_bits(out[k][keep], clean[want][k][keep]), (key, col, k)


# ------------------------------------------------------------------------------ 5. calling conventions
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_calling_conventions(dtype):
    B = 300
    m = _mpc(3, B, dtype)
    a = _dev_case(B, dtype)
    plain = _outs(B, dtype)
    assert _raw(m, B, a, plain) == 0
    torch.cuda.synchronize()
    assert all(bool((plain[k] != 7.0).any()) for k in KEYS)
    # outputs inside sentinel-filled buffers at element-aligned, not 16-byte-aligned bases; inputs too
    isz = plain['gx'].element_size()
    o = {k: ab.guarded((B, COLS[k]), TD[dtype], align=isz) for k in KEYS}
    c = _rows(_case(), B)
    pin = dict(x=ab.padded(c['x'], 12, 1, TD[dtype]), u=ab.padded(c['u'], 4, 3, TD[dtype]),
               g=ab.padded(c['g'], 12, 1, TD[dtype]), wind=ab.padded(c['wind'], 5, 1, TD[dtype]),
               M=ab.padded(c['M'], 17, 3, TD[dtype]))
    assert all(p.ptr % 16 != 0 for p in pin.values())
    assert _raw(m, B, pin, o, model_sb=17, wind_sb=5) == 0
    torch.cuda.synchronize()
    for k in KEYS:
        o[k].check()
        assert ab.same_bits(o[k].view, plain[k]), k
    assert all(p.unchanged() for p in pin.values())
    # gx aliasing gxn
    al = dict(a, g=a['g'].clone())
    assert _raw(m, B, al, dict(gx=al['g'], gu=None, gwind=None, gmodel=None)) == 0
    torch.cuda.synchronize()
    assert ab.same_bits(al['g'], plain['gx'])
    # a non-default stream
    st = torch.cuda.Stream()
    so = _outs(B, dtype)
    st.wait_stream(torch.cuda.current_stream())
    assert _raw(m, B, a, so, stream=st.cuda_stream) == 0
    st.synchronize()
    assert all(ab.same_bits(so[k], plain[k]) for k in KEYS)
    # refusals: nothing is written
    raw = ab.Raw(m)
    ro = _outs(B, dtype)

    def refused(rc_want, B_=B, a_=a, o_=ro, **kw):
        rc = _raw(m, B_, a_, o_, **kw)
        torch.cuda.synchronize()
        assert rc == rc_want, (rc, raw.error(), kw)
        assert all(bool((v == 7.0).all()) for v in ro.values())

    big = {k: (None if v is None else torch.cat([v, v[:1]])) for k, v in a.items()}
    refused(E_INVALID, B_=B + 1, a_=big, o_={k: None for k in KEYS} | {'gx': torch.cat([ro['gx'], ro['gx'][:1]])})
    for k in ('x', 'u', 'g'):
        refused(E_INVALID, a_=dict(a, **{k: None}))
    refused(E_INVALID, o_={})
    refused(E_INVALID, wind_sb=-3)
    refused(E_INVALID, model_sb=-14)
    refused(E_INVALID, model_sb=13)
    refused(E_INVALID, model_sb=1)
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    m17 = BatchedMPC(MPCConfig.full(N=3, dtype=dtype), max_batch=B)
    rc = _raw(m17, B, a, ro)
    torch.cuda.synchronize()
    assert rc == E_UNSUPPORTED and all(bool((v == 7.0).all()) for v in ro.values())
    with pytest.raises(ValueError):
        m17.sim_step_vjp(np.zeros((B, 17)), np.zeros((B, 6)), np.zeros((B, 17)))
    with pytest.raises(ValueError):
        m.sim_step_vjp(c['x'], c['u'], c['g'], want=())
    with pytest.raises(ValueError):
        m.sim_step_vjp(c['x'], c['u'], c['g'], want=('gx', 'gq'))


# ------------------------------------------------------------------------------ 6. sim_step_diff
def test_sim_step_diff():
    B = 5
    m = _mpc(3, B)
    c = _dev_case(B, 'f64')
    lw = torch.as_tensor(np.random.default_rng(9).standard_normal((B, 12)), device='cuda')
    calls = []
    orig = m.sim_step_vjp
    m.sim_step_vjp = lambda *a, **kw: (calls.append(tuple(kw['want'])), orig(*a, **kw))[1]

    def run(x, u, wind, model):
        leaves = [t.clone().requires_grad_(True) if r else t for t, r in (x, u, wind, model)]
        xo = m.sim_step_diff(leaves[0], leaves[1], wind=leaves[2], model=leaves[3])
        (lw * xo).sum().backward()
        return xo, [t.grad if t is not None and t.requires_grad else None for t in leaves]

    # per-instance tensors: the gradients are sim_step_vjp's
    xo, gr = run((c['x'], True), (c['u'], True), (c['wind'], True), (c['M'], True))
    assert calls[-1] == KEYS
    assert ab.same_bits(xo.detach(), m.sim_step(c['x'], c['u'], wind=c['wind'], model=c['M']))
    ref = orig(c['x'], c['u'], lw, wind=c['wind'], model=c['M'], want=KEYS)
    for g, k in zip(gr, KEYS):
        assert ab.same_bits(g, ref[k]), k
    # one row: the batch sums, in the tensor's shape; wider rows: zeros in the pad columns
    w1, M1 = c['wind'][:1].clone(), torch.cat([c['M'][:1], torch.full((1, 2), 3.0, dtype=torch.float64, device='cuda')], 1)
    _, gr = run((c['x'], False), (c['u'], False), (w1, True), (M1, True))
    assert calls[-1] == ('gwind', 'gmodel')
    ref = orig(c['x'], c['u'], lw, wind=w1, model=M1, want=KEYS)
    assert gr[2].shape == (1, 3) and gr[3].shape == (1, 16) and bool((gr[3][:, 14:] == 0).all())
    assert torch.allclose(gr[2], ref['gwind'].sum(0, keepdim=True), rtol=1e-13, atol=0)
    assert torch.allclose(gr[3][:, :14], ref['gmodel'].sum(0, keepdim=True), rtol=1e-13, atol=0)
    _, gr = run((c['x'], False), (c['u'], False), (None, False), (c['M'][0].clone(), True))
    assert calls[-1] == ('gmodel',) and gr[3].shape == (14,)
    # only what is needed is requested
    _, gr = run((c['x'], False), (c['u'], True), (c['wind'], False), (c['M'], False))
    assert calls[-1] == ('gu',) and gr[0] is None
    _, gr = run((c['x'], True), (c['u'], False), (None, False), (None, False))
    assert calls[-1] == ('gx',)
    # a float32 leaf on an f64 handle gets a float32 gradient
    _, gr = run((c['x'].float(), True), (c['u'], False), (c['wind'].float(), True), (None, False))
    assert gr[0].dtype == torch.float32 and gr[2].dtype == torch.float32
    m.sim_step_vjp = orig
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    m17 = BatchedMPC(MPCConfig.full(N=3), max_batch=B)
    with pytest.raises(ValueError):
        m17.sim_step_diff(torch.zeros((B, 17), dtype=torch.float64, device='cuda'),
                          torch.zeros((B, 6), dtype=torch.float64, device='cuda'))


# ------------------------------------------------------------------------------ 7. closed_loop_diff
@pytest.mark.parametrize('box', [True, False])
def test_closed_loop_diff(box):
    """The frozen case of tests/test_simvjp_ref_cpu.py test_frozen_loop_case_of_the_gpu_test, fp64."""
    from mpc_blaster_amd.closed_loop import closed_loop, closed_loop_diff
    case = sr.loop_case(box)
    B, N, nsim = sr.LOOP_B, sr.LOOP_N, sr.LOOP_NSIM
    kw = dict(lbu=sr.LOOP_LB, ubu=sr.LOOP_UB) if box else {}
    m = _mpc(N, B, **kw)
    th = {k: _t(v, 'f64') for k, v in case['theta'].items()}
    xbar, ubar, w = (_t(case[k], 'f64') for k in ('xbar', 'ubar', 'w'))
    wts = lambda t: dict(Q=t['Q'], R=t['R'], QN=t['QN'])   # noqa: E731
    # forward values: closed_loop's, bit for bit.  warm_start=True is closed_loop's persistent iterate;
    # without it every step is closed_loop's single step from the given (xbar, ubar)
    X, U, st = closed_loop_diff(m, th['x0'], th['xref'], th['uref'], nsim, xbar, ubar, weights=wts(th),
                                plant_model=th['plant_model'], warm_start=True)
    Xc, Uc, sc = closed_loop(m, th['x0'], th['xref'], th['uref'], nsim, xbar=xbar, ubar=ubar, weights=wts(th),
                             plant_model=th['plant_model'])
    assert ab.same_bits(X, Xc) and ab.same_bits(U, Uc) and ab.same_bits(st, sc)
    leaves = {k: v.clone().requires_grad_(True) for k, v in th.items()}
    X, U, st = closed_loop_diff(m, leaves['x0'], leaves['xref'], leaves['uref'], nsim, xbar, ubar, weights=wts(leaves),
                                plant_model=leaves['plant_model'], warm_start=False)
    x = th['x0']
    for i in range(nsim):
        Xc, Uc, sc = closed_loop(m, x, th['xref'], th['uref'], 1, xbar=xbar, ubar=ubar, weights=wts(th),
                                 plant_model=th['plant_model'])
        assert ab.same_bits(X[:, i + 1].detach(), Xc[:, 1]) and ab.same_bits(U[:, i].detach(), Uc[:, 0])
        assert int(sc.max()) == 0
        x = Xc[:, 1].contiguous()
    assert int(st.max()) == 0
    # ... and the reference's, so that the quotients below differentiate the same loop
    Lr, Xr, Ur, _, fixed = sr.loop_eval(case, case['theta'])
    assert relerr(X.detach().cpu().numpy(), Xr).max() <= 1e-9
    if box:
        clamped = ((U.detach() <= 5.0) | (U.detach() >= 40.0)).cpu().numpy()
        assert np.array_equal(clamped, fixed[:, :, 0]) and clamped.any()
    # <gradient, direction> against the Richardson quotient of loop_ref
    (w * X).sum().backward()
    quot, same = sr.loop_quotients(case)
    assert same
    bound = max(1e-9, 10.0 * sr.LOOP_SELF[box])
    for d, q in zip(case['dirs'], quot):
        ip = sum(float((leaves[k].grad.cpu().numpy() * d[k]).sum()) for k in sr.LOOP_KEYS)
        e = abs(ip - q) / max(abs(q), 1.0)
        print(f'closed_loop_diff box={box}: <grad, d> {ip:.10g}  quotient {q:.10g}  error {e:.2e}/{bound:.1e}')
        assert e <= bound
