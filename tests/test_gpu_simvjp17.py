"""mpcb_sim_step_p17 / mpcb_sim_step_vjp17 on the GPU (the 17/6 plant step with the plant's parameters
as an argument, and its reverse mode), ``sim_step_diff17``, ``closed_loop(plant_params=)`` and
``closed_loop_diff`` on the 17/6 model, against tests/simvjp17_ref.py: the device is compared with the
NumPy reference, which tests/test_simvjp17_ref_cpu.py ties to central differences of the oracle.

Metric: per instance and per block (gx, gu, gJ = gparams[:24], gtb = gparams[24])
|dev - ref|_inf / |ref|_inf over the block (tests/simvjp17_ref.py ``blockerr``): no floor of 1, which
would hide the parameter gradients (about 1e-2); the CPU test holds every block of the frozen draw
to |ref|_inf >= 1e-4.  Bounds: fp64 1e-9.  fp32 by the rule of tests/test_gpu_simvjp.py: the reference
reads fp32-rounded inputs, its own move under a seeded +-2^-22 relative perturbation of every input is
measured, and the device is held to max(5e-5, 10 x move), per block.  Shapes: B = 1, 5 and 70 (more
than one 64-thread block, the last one partial).  Draw: tests/simvjp17_ref.py ``step_case``.  Each
test prints its measured maxima (DESIGN.md records them).
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_call as ab   # noqa: E402
import simvjp17_ref as s17   # noqa: E402
import vjp17_ref as vr   # noqa: E402

from oracle.full import default_p25   # noqa: E402
from oracle.model import Params   # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

KEYS = ('gx', 'gu', 'gparams')
COLS = dict(gx=17, gu=6, gparams=25)
TD = {'f64': torch.float64, 'f32': torch.float32}
BOUND = {'f64': 1e-9, 'f32': 5e-5}
SHAPES = s17.SHAPES
BMAX = s17.BMAX
E_INVALID, E_UNSUPPORTED = -1, -4
T = 2.0 / 60.0
P = Params()
WANTS = [(k,) for k in KEYS] + [('gx', 'gu'), ('gu', 'gparams'), KEYS]


def _mpc(N, B, dtype='f64', **kw):
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    return BatchedMPC(MPCConfig.full(N=N, dtype=dtype, **kw), max_batch=B)


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _pert(rng, a):
    return a * (1.0 + 2.0 ** -22 * rng.choice([-1.0, 1.0], size=np.shape(a)))


@functools.lru_cache(maxsize=None)
def _case():
    c = s17.step_case()
    for a in c.values():
        a.setflags(write=False)
    return c


def _rows(B):
    return {k: v[:B] for k, v in _case().items()}


@functools.lru_cache(maxsize=None)
def _ref(dtype, params='pi'):
    """(reference blocks at BMAX instances, the per-block bound); computed once per variant and
    shared, instance b's row does not depend on B.  params: 'pi' per instance, 'bc' the first row
    broadcast, 'def' the defaults."""
    c = dict(_case())
    c['p'] = dict(pi=c['p'], bc=c['p'][:1], **{'def': default_p25()[None]})[params]
    if dtype == 'f32':
        c = {k: _f32(v) for k, v in c.items()}
    ref = s17.blocks(s17.simvjp17_ref(c['x'], c['u'], c['g'], T, P, c['p']))
    bound = {k: BOUND['f64'] for k in s17.BLOCKS}
    if dtype == 'f32':
        rng = np.random.default_rng(0)
        q = {k: _pert(rng, v) for k, v in c.items()}
        moved = s17.blocks(s17.simvjp17_ref(q['x'], q['u'], q['g'], T, P, q['p']))
        move = {k: s17.blockerr(moved[k], ref[k]).max() for k in s17.BLOCKS}
        bound = {k: max(BOUND['f32'], 10.0 * move[k]) for k in s17.BLOCKS}
        print(f'fp32 reference move ({params}): ' + '  '.join(f'{k} {move[k]:.2e}' for k in s17.BLOCKS))
    return ref, bound


def _t(a, dtype):
    return None if a is None else torch.as_tensor(np.array(a), dtype=TD[dtype], device='cuda')


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}


def _check(got, ref, bound, B, tag, keys=KEYS):
    for k in keys:
        assert got[k].shape == (B, COLS[k]), (tag, k)
    gb = s17.blocks(got)
    err = {k: s17.blockerr(gb[k], ref[k][:B]).max() for k in gb}
    print(f'{tag}: ' + '  '.join(f'{k} {err[k]:.2e}/{bound[k]:.1e}' for k in gb))
    for k in gb:
        assert err[k] <= bound[k], (tag, k, err[k], bound[k])


def _raw(m, B, a, o, params_sb=None, T_=T, stream=0):
    """mpcb_sim_step_vjp17 with pointers and strides as given; a: x, u, g, p; o: the three outputs
    (missing / None = NULL)."""
    if params_sb is None:
        params_sb = 25 if a.get('p') is not None else 0
    return m.lib.mpcb_sim_step_vjp17(m._h, B, ab._p(a['x']), ab._p(a['u']), ab._p(a.get('p')), params_sb, float(T_),
                                     ab._p(a['g']), *(ab._p(o.get(k)) for k in KEYS), ab._p(stream))


def _dev_case(B, dtype):
    return {k: _t(v, dtype) for k, v in _rows(B).items()}


def _outs(B, dtype, keys=KEYS):
    return {k: torch.full((B, COLS[k]), 7.0, dtype=TD[dtype], device='cuda') for k in keys}


# ------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('B', SHAPES)
def test_all_outputs_match_reference(dtype, B):
    m = _mpc(3, B, dtype)
    c = _rows(B)
    call = lambda **kw: _np(m.sim_step_vjp17(c['x'], c['u'], c['g'], T=T, want=KEYS, **kw))   # noqa: E731
    # NULL with the defaults
    ref, bound = _ref(dtype, 'def')
    _check(call(), ref, bound, B, f'{dtype} B={B} defaults')
    # per-instance parameter vectors
    ref, bound = _ref(dtype)
    _check(call(params=c['p']), ref, bound, B, f'{dtype} B={B} per-instance')
    # stride 27 with NaN in the pad
    got = call(params=np.concatenate([c['p'], np.full((B, 2), np.nan)], axis=1))
    assert all(np.isfinite(v).all() for v in got.values())
    _check(got, ref, bound, B, f'{dtype} B={B} params_sb=27')
    # NULL after set_params: the handle's rows at stage 0
    m.set_params(c['p'])
    _check(call(), ref, bound, B, f'{dtype} B={B} set_params rows')
    # one vector for all: rows per instance, the reference at the broadcast vector; it wins over set_params
    ref, bound = _ref(dtype, 'bc')
    _check(call(params=c['p'][:1]), ref, bound, B, f'{dtype} B={B} broadcast')
    _check(call(params=c['p'][0]), ref, bound, B, f'{dtype} B={B} broadcast [25]')


# ------------------------------------------------------------------------------ 2. output selection
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_output_selection_and_reproducibility(dtype):
    B = BMAX
    m = _mpc(3, B, dtype)
    c = _rows(B)
    for params in (c['p'], None):
        call = lambda want: m.sim_step_vjp17(c['x'], c['u'], c['g'], T=T, params=params, want=want)   # noqa: E731
        full = call(KEYS)
        for want in WANTS:
            out = call(want)
            torch.cuda.synchronize()
            assert tuple(out) == tuple(want)
            for k in want:
                assert ab.same_bits(out[k], full[k]), (want, k)
        again = call(KEYS)
        torch.cuda.synchronize()
        assert all(ab.same_bits(full[k], again[k]) for k in KEYS)


# ------------------------------------------------------------------------------ 3./4. the forward kernels
def test_consistent_with_linearize_and_sim_step_unchanged():
    B = BMAX
    c = _rows(B)
    m = _mpc(1, B)   # N = 1: linearize gives one [A | B] per instance at (x, u)
    x, u, g, p = (_t(c[k], 'f64') for k in ('x', 'u', 'g', 'p'))
    before_def = m.sim_step(x, u, T=T).clone()
    with_arg = m.sim_step(x, u, T=T, params=p).clone()
    with_arg_bc = m.sim_step(x, u, T=T, params=p[:1]).clone()
    m.set_params(c['p'])
    xbar = torch.stack([x, x], dim=1).contiguous()
    A, Bm, _ = m.linearize(xbar, u.unsqueeze(1).contiguous())
    before = m.sim_step(x, u, T=T).clone()
    got = m.sim_step_vjp17(x, u, g, T=m.cfg.dt, want=KEYS)
    ex = torch.einsum('bij,bi->bj', A[:, 0], g)
    eu = torch.einsum('bij,bi->bj', Bm[:, 0], g)
    e = (s17.blockerr(got['gx'].cpu().numpy(), ex.cpu().numpy()).max(),
         s17.blockerr(got['gu'].cpu().numpy(), eu.cpu().numpy()).max())
    print(f'against the device\'s own linearize at N = 1: gx {e[0]:.2e}  gu {e[1]:.2e} / 1e-9')
    assert max(e) <= 1e-9
    # sim_step returns the same bits before and after; sim_step(params=P) is set_params(P) + sim_step
    m.sim_step_vjp17(x, u, g, T=T, params=p, want=KEYS)
    assert ab.same_bits(before, m.sim_step(x, u, T=T))
    assert ab.same_bits(before, with_arg)
    assert ab.same_bits(m.sim_step(x, u, T=T, params=p), with_arg)
    m.set_params(c['p'][:1])
    assert ab.same_bits(m.sim_step(x, u, T=T), with_arg_bc)
    m.set_params(None)
    assert ab.same_bits(m.sim_step(x, u, T=T), before_def)
    m12 = _mpc12(B)
    with pytest.raises(ValueError):
        m12.sim_step(np.zeros((B, 12)), np.zeros((B, 4)), params=c['p'])


def _mpc12(B, dtype='f64'):
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    return BatchedMPC(MPCConfig(N=3, dtype=dtype), max_batch=B)


# ------------------------------------------------------------------------------ 5. the NaN rule
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_nan_rule(dtype):
    B, bad = BMAX, 66   # in the last, partial block
    m = _mpc(3, B, dtype)
    c = _rows(B)
    wants = (KEYS, ('gu',), ('gx', 'gu'), ('gparams',))
    # (the clean run of the same request: the gx / gu-only kernel is another instantiation)
    clean = {w: m.sim_step_vjp17(c['x'], c['u'], c['g'], T=T, params=c['p'], want=w) for w in wants}
    keep = torch.arange(B, device='cuda') != bad
    # x[0], x[15] enter no derivative and gxn[0] only gx[0]: the check sum alone carries those
    for key, col in (('x', 0), ('x', 4), ('x', 15), ('u', 2), ('u', 5), ('g', 0), ('p', 3), ('p', 24)):
        a = {k: v.copy() for k, v in c.items()}
        a[key][bad, col] = np.nan
        for want in wants:
            out = m.sim_step_vjp17(a['x'], a['u'], a['g'], T=T, params=a['p'], want=want)
            torch.cuda.synchronize()
            for k in want:
                assert bool(torch.isnan(out[k][bad]).all()), (key, col, k)
                assert ab.same_bits(out[k][keep], clean[want][k][keep]), (key, col, k)


# ------------------------------------------------------------------------------ 6. calling conventions
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_calling_conventions(dtype):
    B = BMAX
    m = _mpc(3, B, dtype)
    a = _dev_case(B, dtype)
    plain = _outs(B, dtype)
    assert _raw(m, B, a, plain) == 0
    torch.cuda.synchronize()
    assert all(bool((plain[k] != 7.0).any()) for k in KEYS)
    # outputs inside sentinel-filled buffers at element-aligned, not 16-byte-aligned bases; inputs too
    isz = plain['gx'].element_size()
    o = {k: ab.guarded((B, COLS[k]), TD[dtype], align=isz) for k in KEYS}
    c = _rows(B)
    pin = dict(x=ab.padded(c['x'], 17, 1, TD[dtype]), u=ab.padded(c['u'], 6, 3, TD[dtype]),
               g=ab.padded(c['g'], 17, 1, TD[dtype]), p=ab.padded(c['p'], 27, 3, TD[dtype]))
    assert all(q.ptr % 16 != 0 for q in pin.values())
    assert _raw(m, B, pin, o, params_sb=27) == 0
    torch.cuda.synchronize()
    for k in KEYS:
        o[k].check()
        assert ab.same_bits(o[k].view, plain[k]), k
    assert all(q.unchanged() for q in pin.values())
    # gx aliasing gxn
    al = dict(a, g=a['g'].clone())
    assert _raw(m, B, al, dict(gx=al['g'])) == 0
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

    def refused(rc_want, m_=m, B_=B, a_=a, o_=ro, **kw):
        rc = _raw(m_, B_, a_, o_, **kw)
        torch.cuda.synchronize()
        assert rc == rc_want, (rc, raw.error(), kw)
        assert all(bool((v == 7.0).all()) for v in ro.values())

    big = {k: torch.cat([v, v[:1]]) for k, v in a.items()}
    refused(E_INVALID, B_=B + 1, a_=big, o_={'gx': torch.cat([ro['gx'], ro['gx'][:1]])})
    for k in ('x', 'u', 'g'):
        refused(E_INVALID, a_=dict(a, **{k: None}))
    refused(E_INVALID, o_={})
    refused(E_INVALID, params_sb=-25)
    refused(E_INVALID, params_sb=24)
    refused(E_INVALID, params_sb=1)
    refused(E_INVALID, T_=0.0)
    refused(E_INVALID, T_=-T)
    # params == NULL with a non-broadcast set_params array shorter than B; a broadcast one is fine
    m.set_params(c['p'][:B - 1])
    refused(E_INVALID, a_=dict(a, p=None))
    m.set_params(c['p'][:1])
    assert _raw(m, B, dict(a, p=None), _outs(B, dtype)) == 0
    m.set_params(None)
    # a 12/4 handle
    m12 = _mpc12(B, dtype)
    refused(E_UNSUPPORTED, m_=m12)
    xo = torch.full((B, 17), 7.0, dtype=TD[dtype], device='cuda')
    rc = m12.lib.mpcb_sim_step_p17(m12._h, B, ab._p(a['x']), ab._p(a['u']), ab._p(a['p']), 25, T, ab._p(xo), ab._p(0))
    torch.cuda.synchronize()
    assert rc == E_UNSUPPORTED and bool((xo == 7.0).all())
    for sb in (-25, 24):
        rc = m.lib.mpcb_sim_step_p17(m._h, B, ab._p(a['x']), ab._p(a['u']), ab._p(a['p']), sb, T, ab._p(xo), ab._p(0))
        torch.cuda.synchronize()
        assert rc == E_INVALID and bool((xo == 7.0).all())
    with pytest.raises(ValueError):
        m12.sim_step_vjp17(np.zeros((B, 12)), np.zeros((B, 4)), np.zeros((B, 12)))
    with pytest.raises(ValueError):
        m12.sim_step_diff17(torch.zeros((B, 12), dtype=TD[dtype], device='cuda'),
                            torch.zeros((B, 4), dtype=TD[dtype], device='cuda'))
    with pytest.raises(ValueError):
        m.sim_step_vjp17(c['x'], c['u'], c['g'], want=())
    with pytest.raises(ValueError):
        m.sim_step_vjp17(c['x'], c['u'], c['g'], want=('gx', 'gmodel'))
    with pytest.raises(ValueError):
        m.sim_step_vjp17(c['x'], c['u'], c['g'], params=c['p'][:, :24])
    with pytest.raises(ValueError):
        m.sim_step_vjp17(c['x'], c['u'], c['g'], params=c['p'][:2])


# ------------------------------------------------------------------------------ 7. sim_step_diff17
def test_sim_step_diff17():
    B = 5
    m = _mpc(3, B)
    c = _dev_case(B, 'f64')
    lw = torch.as_tensor(np.random.default_rng(9).standard_normal((B, 17)), device='cuda')
    calls = []
    orig = m.sim_step_vjp17
    m.sim_step_vjp17 = lambda *a, **kw: (calls.append(tuple(kw['want'])), orig(*a, **kw))[1]

    def run(x, u, params):
        leaves = [t.clone().requires_grad_(True) if r else t for t, r in (x, u, params)]
        xo = m.sim_step_diff17(leaves[0], leaves[1], T=T, params=leaves[2])
        loss = (lw * xo).sum()
        return xo, loss, leaves

    def grads(x, u, params):
        xo, loss, leaves = run(x, u, params)
        loss.backward()
        return xo, [t.grad if t is not None and t.requires_grad else None for t in leaves]

    # per-instance tensors: the gradients are sim_step_vjp17's
    xo, gr = grads((c['x'], True), (c['u'], True), (c['p'], True))
    assert calls[-1] == KEYS
    assert ab.same_bits(xo.detach(), m.sim_step(c['x'], c['u'], T=T, params=c['p']))
    ref = orig(c['x'], c['u'], lw, T=T, params=c['p'], want=KEYS)
    for g, k in zip(gr, KEYS):
        assert ab.same_bits(g, ref[k]), k
    # one row: the batch sum, in the tensor's shape; wider rows: zeros in the pad columns
    p1 = torch.cat([c['p'][:1], torch.full((1, 2), 3.0, dtype=torch.float64, device='cuda')], 1)
    _, gr = grads((c['x'], False), (c['u'], False), (p1, True))
    assert calls[-1] == ('gparams',)
    ref = orig(c['x'], c['u'], lw, T=T, params=p1, want=KEYS)
    assert gr[2].shape == (1, 27) and bool((gr[2][:, 25:] == 0).all())
    assert torch.allclose(gr[2][:, :25], ref['gparams'].sum(0, keepdim=True), rtol=1e-13, atol=0)
    _, gr = grads((c['x'], False), (c['u'], False), (c['p'][0].clone(), True))
    assert calls[-1] == ('gparams',) and gr[2].shape == (25,)
    assert torch.allclose(gr[2], orig(c['x'], c['u'], lw, T=T, params=c['p'][:1], want=KEYS)['gparams'].sum(0),
                          rtol=1e-13, atol=0)
    # only what is needed is requested
    _, gr = grads((c['x'], False), (c['u'], True), (c['p'], False))
    assert calls[-1] == ('gu',) and gr[0] is None
    _, gr = grads((c['x'], True), (c['u'], False), (None, False))
    assert calls[-1] == ('gx',)
    # a float32 leaf on an f64 handle gets a float32 gradient
    _, gr = grads((c['x'].float(), True), (c['u'], False), (c['p'][:1].float(), True))
    assert gr[0].dtype == torch.float32 and gr[2].dtype == torch.float32 and gr[2].shape == (1, 25)
    # set_params between forward and backward raises only when params was not given
    _, loss, _ = run((c['x'], True), (c['u'], True), (None, False))
    m.set_params(c['p'])
    with pytest.raises(RuntimeError, match='set_params'):
        loss.backward()
    _, loss, _ = run((c['x'], True), (c['u'], True), (None, False))
    m.set_t_blast(20.0)
    with pytest.raises(RuntimeError, match='set_t_blast'):
        loss.backward()
    _, loss, leaves = run((c['x'], True), (c['u'], True), (c['p'], True))
    m.set_params(None)
    loss.backward()
    assert ab.same_bits(leaves[0].grad, orig(c['x'], c['u'], lw, T=T, params=c['p'], want=('gx',))['gx'])
    m.sim_step_vjp17 = orig


# ------------------------------------------------------------------------------ 8. call history
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_results_do_not_depend_on_the_call_history(dtype):
    B, N = 5, 3
    c = _rows(B)
    fresh = _mpc(N, B, dtype)
    fresh.set_params(c['p'])
    want_arg = fresh.sim_step_vjp17(c['x'], c['u'], c['g'], T=T, params=c['p'], want=KEYS)
    want_null = fresh.sim_step_vjp17(c['x'], c['u'], c['g'], T=T, want=KEYS)
    m = _mpc(N, B, dtype)
    v = vr.vjp17_case(B, N)
    m.solve_iterate(v['x0'], v['xbar'], v['ubar'], v['xref'], v['uref'])
    m.set_params(v['p'])
    m.solve_iterate_vjp(v['xbar'], v['ubar'], gX=v['gX'], gU=v['gU'])
    m.sim_step(c['x'], c['u'], T=T)
    m.sim_step(c['x'], c['u'], T=T, params=c['p'][:1])
    got = m.sim_step_vjp17(c['x'], c['u'], c['g'], T=T, params=c['p'], want=KEYS)
    m.set_params(c['p'])
    got_null = m.sim_step_vjp17(c['x'], c['u'], c['g'], T=T, want=KEYS)
    torch.cuda.synchronize()
    for k in KEYS:
        assert ab.same_bits(got[k], want_arg[k]) and ab.same_bits(got_null[k], want_null[k]), k
        assert ab.same_bits(want_arg[k], want_null[k]), k


# ------------------------------------------------------------------------------ 9. closed_loop(plant_params=)
@pytest.mark.parametrize('held', [False, True])
def test_closed_loop_plant_params(held):
    from mpc_blaster_amd.closed_loop import closed_loop
    case = s17.loop17_case(True)
    B, N, nsim = s17.LOOP17_B, s17.LOOP17_N, s17.LOOP17_NSIM
    th = case['theta']
    m = _mpc(N, B, lbu=vr.LBU17, ubu=vr.UBU17)
    m.set_params(case['p'])
    kw = dict(resolve_every=2) if held else {}
    # plant_params equal to the set_params rows: the bits of the loop without it
    Xa, Ua, sa = closed_loop(m, th['x0'], th['xref'], th['uref'], nsim, xbar=case['xbar'], ubar=case['ubar'], **kw)
    Xb, Ub, sb = closed_loop(m, th['x0'], th['xref'], th['uref'], nsim, xbar=case['xbar'], ubar=case['ubar'],
                             plant_params=case['p'], **kw)
    torch.cuda.synchronize()
    assert ab.same_bits(Xa, Xb) and ab.same_bits(Ua, Ub) and ab.same_bits(sa, sb)
    Xs, Us, st = closed_loop(m, th['x0'], th['xref'], th['uref'], nsim, xbar=case['xbar'], ubar=case['ubar'],
                             plant_params=th['plant_params'], **kw)
    torch.cuda.synchronize()
    assert not ab.same_bits(Xs, Xa)   # the plant does fly other parameters
    m12 = _mpc12(B)
    with pytest.raises(ValueError):
        closed_loop(m12, np.zeros((B, 12)), np.zeros((1, 4, 12)), np.zeros((1, 3, 4)), 1, plant_params=case['p'], **kw)
    if held:
        return
    # against loop17_ref (the persistent iterate) at the closed-loop bound of tests/test_gpu_full17.py
    Xr, Ur, sr_, _ = s17.loop17_ref(th['x0'], th['xref'], th['uref'], nsim, case['xbar'], case['ubar'], case['spec'],
                                    case['p'], th['plant_params'], warm_start=True)
    Xs, Us = Xs.cpu().numpy(), Us.cpu().numpy()
    eu = max(vr.relerr(Us[:, i], Ur[:, i]).max() for i in range(nsim))
    ex = max(vr.relerr(Xs[:, i], Xr[:, i]).max() for i in range(nsim + 1))
    print(f'closed_loop(plant_params=) against loop17_ref: u0 {eu:.2e} x {ex:.2e} / 1e-5')
    assert np.array_equal(st.cpu().numpy(), sr_)
    assert eu <= 1e-5 and ex <= 1e-5


# ------------------------------------------------------------------------------ 10. closed_loop_diff on 17/6
@pytest.mark.parametrize('box', [True, False])
def test_closed_loop_diff17(box):
    """The frozen case of tests/test_simvjp17_ref_cpu.py test_frozen_loop_case_of_the_gpu_test, fp64:
    <grad, d> against the Richardson quotient of loop17_ref.  Bound: max(1e-9, 10 x the quotients'
    self-agreement) and, with the box, also 10 K delta: the device's interior point and the oracle's
    need not return the same u0, so the adjoint runs at slightly different points; delta is the
    deviation of the device's U_sim from the oracle's measured in this run (held to 1e-9, the bound
    tests/test_gpu_full17.py gives the fp64 input-box solve) and K the move of the quotients per unit
    of it (tests/simvjp17_ref.py LOOP17_K).  The quotient of the oracle's interior-point loop is itself
    only that close to the derivative on the active set (LOOP17_GAP, measured on the CPU: 2.0e-10 with
    the box), so the gradient is also held to the NumPy adjoint of the same loop at 1e-9.
    Measured: delta 1.9e-15; error against the quotients 2.0e-10 (box) and 6.3e-11; against the
    reference adjoint 1e-15."""
    from mpc_blaster_amd.closed_loop import closed_loop, closed_loop_diff
    case = s17.loop17_case(box)
    B, N, nsim = s17.LOOP17_B, s17.LOOP17_N, s17.LOOP17_NSIM
    kw = dict(lbu=vr.LBU17, ubu=vr.UBU17) if box else {}
    m = _mpc(N, B, **kw)
    m.set_params(case['p'])
    th = {k: _t(v, 'f64') for k, v in case['theta'].items()}
    xbar, ubar, w = (_t(case[k], 'f64') for k in ('xbar', 'ubar', 'w'))
    # forward values: closed_loop's, bit for bit.  warm_start=True is closed_loop's persistent iterate;
    # without it every step is closed_loop's single step from the given (xbar, ubar)
    X, U, st = closed_loop_diff(m, th['x0'], th['xref'], th['uref'], nsim, xbar, ubar,
                                plant_params=th['plant_params'], warm_start=True)
    Xc, Uc, sc = closed_loop(m, th['x0'], th['xref'], th['uref'], nsim, xbar=xbar, ubar=ubar,
                             plant_params=th['plant_params'])
    assert ab.same_bits(X, Xc) and ab.same_bits(U, Uc) and ab.same_bits(st, sc)
    leaves = {k: v.clone().requires_grad_(True) for k, v in th.items()}
    X, U, st = closed_loop_diff(m, leaves['x0'], leaves['xref'], leaves['uref'], nsim, xbar, ubar,
                                plant_params=leaves['plant_params'], warm_start=False)
    x = th['x0']
    for i in range(nsim):
        Xc, Uc, sc = closed_loop(m, x, th['xref'], th['uref'], 1, xbar=xbar, ubar=ubar, plant_params=th['plant_params'])
        assert ab.same_bits(X[:, i + 1].detach(), Xc[:, 1]) and ab.same_bits(U[:, i].detach(), Uc[:, 0])
        assert int(sc.max()) == 0
        x = Xc[:, 1].contiguous()
    assert int(st.max()) == 0
    # ... and the reference's, so that the quotients below differentiate the same loop
    _, Xr, Ur, _, fixed = s17.loop17_eval(case, case['theta'])
    delta = float(vr.relerr(U.detach().cpu().numpy(), Ur).max())
    ex = float(vr.relerr(X.detach().cpu().numpy(), Xr).max())
    print(f'closed_loop_diff 17/6 box={box}: U_sim against the oracle delta = {delta:.2e}/1e-9, X_sim {ex:.2e}/1e-9')
    assert delta <= 1e-9 and ex <= 1e-9
    if box:
        clamped = m.active_mask17(U.detach().unsqueeze(2)).squeeze(2).cpu().numpy().astype(bool)
        assert np.array_equal(clamped, fixed[:, :, 0]) and clamped.any() and not clamped.all()
    # <gradient, direction> against the Richardson quotient of loop17_ref
    (w * X).sum().backward()
    quot, same = s17.loop17_quotients(case)
    assert same
    bound = max(1e-9, 10.0 * s17.LOOP17_SELF[box], 10.0 * s17.LOOP17_K * delta if box else 0.0)
    print(f'bound {bound:.2e} = max(1e-9, 10 x self-agreement {s17.LOOP17_SELF[box]:.1e}'
          + (f', 10 x K {s17.LOOP17_K} x delta {delta:.2e})' if box else ')'))
    gref = s17.loop17_grad_ref(case)
    for d, q in zip(case['dirs'], quot):
        ip = sum(float((leaves[k].grad.cpu().numpy() * d[k]).sum()) for k in s17.LOOP17_KEYS)
        e = abs(ip - q) / max(abs(q), 1.0)
        print(f'closed_loop_diff 17/6 box={box}: <grad, d> {ip:.10g}  quotient {q:.10g}  error {e:.2e}/{bound:.1e}')
        assert e <= bound
        # ... and against the reference's own adjoint, which has no interior-point gap (LOOP17_GAP)
        ir = sum(float((gref[k] * d[k]).sum()) for k in s17.LOOP17_KEYS)
        er = abs(ip - ir) / max(abs(ir), 1.0)
        print(f'closed_loop_diff 17/6 box={box}: reference adjoint {ir:.10g}  error {er:.2e}/1e-9')
        assert er <= 1e-9
    for k in s17.LOOP17_KEYS:
        ek = float(vr.relerr(leaves[k].grad.cpu().numpy(), gref[k]).max())
        print(f'closed_loop_diff 17/6 box={box}: gradient of {k} against the reference adjoint {ek:.2e}/1e-9')
        assert ek <= 1e-9
    # a one-row plant_params receives the batch sum in its own shape
    p1 = th['plant_params'][:1].clone().requires_grad_(True)
    X1, _, _ = closed_loop_diff(m, th['x0'], th['xref'], th['uref'], nsim, xbar, ubar, plant_params=p1, warm_start=False)
    (w * X1).sum().backward()
    assert p1.grad.shape == (1, 25) and bool(torch.isfinite(p1.grad).all())
    # refusals
    for bad in (dict(weights=dict(Q=torch.ones((1, 17), dtype=torch.float64, device='cuda'))),
                dict(plant_model=torch.ones((1, 14), dtype=torch.float64, device='cuda')),
                dict(wind=torch.zeros((1, 3), dtype=torch.float64, device='cuda'))):
        with pytest.raises(ValueError):
            closed_loop_diff(m, th['x0'], th['xref'], th['uref'], nsim, xbar, ubar, **bad)
    if box:
        mx = _mpc(N, B, lbu=vr.LBU17, ubu=vr.UBU17, lbx=np.full(17, -10.0), ubx=np.full(17, 10.0))
        with pytest.raises(ValueError):
            closed_loop_diff(mx, th['x0'], th['xref'], th['uref'], nsim, xbar, ubar)
    else:
        m12 = _mpc12(B)
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device='cuda')   # noqa: E731
        for bad in (dict(plant_params=th['plant_params']), dict(active_tol=1e-6)):
            with pytest.raises(ValueError):
                closed_loop_diff(m12, z(B, 12), z(1, N + 1, 12), z(1, N, 4), 1, z(B, N + 1, 12), z(B, N, 4), **bad)
