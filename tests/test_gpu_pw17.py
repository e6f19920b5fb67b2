"""Per-instance cost weights on the 17/6 model on the GPU: mpcb_solve_iterate_pw17, mpcb_solve_vjp_pw17,
the torch layer and the closed loops, against tests/pw17_ref.py (the oracle's mpc_solve17 and
tests/vjp17_ref.py instance by instance with that instance's matrices).  tests/test_pw17_ref_cpu.py
ties that reference to the batched oracle and to finite differences in the weights.

Metric: tests/vjp17_ref.py ``relerr``, per instance |dev - ref|_inf / max(|ref|_inf, 1).

Bounds.  fp64 without the box: 1e-9 (every fp64 17/6 solve test).  With a box the interior point
stops where its tolerances let it, so instance b is held to max(1e-9, 2 e_shared(b)): e_shared(b) is
the error, against the same oracle, of ``solve_iterate`` on a second handle created with instance
b's weights, i.e. the shared-weight kernel on the same problem; the factor 2 allows for another
rounding order and nothing more.  fp32: u0 within max(5e-4 without the box / 1e-3 with the input
box, 2 e_shared(b)), the bounds of test_solve17_fp32_* with the same second-handle measurement.  The
product: tests/test_gpu_vjp17.py's 1e-9 / 5e-4.

Shapes: B = 6 (not a multiple of the four groups of a wave, so the last wave carries padding groups),
N = 6 and 8; B = 70 under MPCB_CHUNK = 64 for the chunk seam and a ragged second chunk.
"""
import ctypes
import functools
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pw17_ref as pr    # noqa: E402
import vjp17_ref as vr   # noqa: E402

from oracle.full import FullSpec   # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

KEYS, WKEYS, WN = vr.KEYS, vr.WKEYS, pr.WNAMES
OUT = ('u0', 'X', 'U')
VBOUND = {'f64': 1e-9, 'f32': 5e-4}           # tests/test_gpu_vjp17.py BOUND
F32_U0 = {'none': 5e-4, 'input': 1e-3}        # test_solve17_fp32_close_to_fp64_oracle, ..._input_box_...
E_UNSUPPORTED, E_INVALID = -4, -1
SIGMA = 0.7


# ------------------------------------------------------------------------------ draws and references (shared)
def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _sbox_inputs(B, N, seed):
    """tests/test_gpu_full17.py _sbox_inputs: x0 inside a quarter of the reference's state box."""
    d = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'ocp_json_pin.json')))
    lbx, ubx = np.array(d['lbx']), np.array(d['ubx'])
    x0, xref, uref, p = vr.inputs17(B, N, seed)
    rng = np.random.default_rng(seed + 1)
    x0 = rng.uniform(0.25 * lbx, 0.25 * ubx, (B, 17))
    x0[:, 2] = 3.5 + rng.uniform(-0.5, 0.5, B)
    return x0, xref, uref, p, lbx, ubx


@functools.lru_cache(maxsize=None)
def _draw(box, B=6):
    """(spec, case, weights dict, handle keywords) of a box mode: 'none' vjp17_case(B, 6), 'input'
    boxed_case(B, 6), 'state' the _sbox_inputs draw at (B, 8) in iterate mode."""
    if box == 'none':
        spec = FullSpec(N=6)
        c, kw = vr.vjp17_case(B, 6, spec), {}
    elif box == 'input':
        spec, c = vr.boxed_case(B, 6)
        kw = dict(lbu=vr.LBU17, ubu=vr.UBU17)
    else:
        N = 8
        x0, xref, uref, p, lbx, ubx = _sbox_inputs(B, N, 41)
        rng = np.random.default_rng(42)
        c = dict(x0=x0, xref=xref, uref=uref, p=p, xbar=x0[:, None, :] + rng.normal(0, 0.01, (B, N + 1, 17)),
                 ubar=uref + rng.normal(0, 0.5, (B, N, 6)))
        kw = dict(lbu=vr.LBU17, ubu=vr.UBU17, lbx=lbx, ubx=ubx)
        spec = FullSpec(N=N, **kw)
    W = dict(zip(WN, pr.pw17_weights(B, spec, SIGMA)))
    return spec, _freeze(c), _freeze(W), kw


@functools.lru_cache(maxsize=None)
def _solve_ref(box, B=6):
    spec, c, W, _ = _draw(box, B)
    return _freeze(pr.pw17_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, c['p'], **W))


def _mpc(N, B, dtype='f64', **kw):
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    return BatchedMPC(MPCConfig.full(N=N, dtype=dtype, **kw), max_batch=B)


def _handle(box, dtype='f64', B=6, **more):
    spec, c, _, kw = _draw(box, B)
    m = _mpc(spec.N, B, dtype, **kw, **more)
    m.set_params(c['p'])
    return m


def _outs(m):
    torch.cuda.synchronize()
    return dict(u0=m.get_control().cpu().numpy().astype(np.float64),
                X=m.get_state_trajectory().cpu().numpy().astype(np.float64),
                U=m.get_input_trajectory().cpu().numpy().astype(np.float64),
                status=m.get_status().cpu().numpy())


def _pw(m, c, W, rows=slice(None)):
    m.solve_iterate_pw17(c['x0'][rows], c['xbar'][rows], c['ubar'][rows], c['xref'][rows], c['uref'][rows],
                         **{k: (None if v is None else v[rows]) for k, v in W.items()})
    return _outs(m)


def _shared(m, c, rows=slice(None)):
    m.solve_iterate(c['x0'][rows], c['xbar'][rows], c['ubar'][rows], c['xref'][rows], c['uref'][rows])
    return _outs(m)


def _err(got, ref, keys=OUT):
    """Per instance, the largest relerr over the outputs."""
    return np.max([vr.relerr(got[k], ref[k]) for k in keys], axis=0)


def _e_shared(box, dtype, keys=OUT, B=6, rows=None):
    """Per instance b of ``rows``: (error against the oracle, status) of solve_iterate on a handle created
    with instance b's weights, which is the shared-weight kernel on the same problem."""
    spec, c, W, kw = _draw(box, B)
    ref = _solve_ref(box, B) if B == 6 else None
    e, st = [], []
    for b in (range(B) if rows is None else rows):
        mb = _mpc(spec.N, 1, dtype, **kw, **{k: W[k][b] for k in WN})
        mb.set_params(c['p'][b:b + 1])
        g = _shared(mb, c, slice(b, b + 1))
        rb = ref if ref is not None else _ref_rows(box, B, tuple(rows))
        i = b if ref is not None else list(rows).index(b)
        e.append(_err(g, {k: rb[k][i:i + 1] for k in OUT}, keys)[0])
        st.append(g['status'][0])
        mb.close()
    return np.array(e), np.array(st)


@functools.lru_cache(maxsize=None)
def _ref_rows(box, B, rows):
    spec, c, W, _ = _draw(box, B)
    r = list(rows)
    return _freeze(pr.pw17_solve_ref(c['x0'][r], c['xref'][r], c['uref'][r], c['xbar'][r], c['ubar'][r], spec,
                                     c['p'][r], **{k: v[r] for k, v in W.items()}))


# ------------------------------------------------------------------------------ 1. solve parity, fp64, no box
def test_solve_fp64_no_box_matches_reference_and_sees_the_weights():
    spec, c, W, _ = _draw('none')
    ref = _solve_ref('none')
    m = _handle('none')
    got = _pw(m, c, W)
    e = {k: vr.relerr(got[k], ref[k]).max() for k in OUT}
    print('pw17 fp64 no box: ' + '  '.join(f'{k} {v:.2e}' for k, v in e.items()))
    assert np.array_equal(got['status'], ref['status']) and (ref['status'] == 0).all()
    assert max(e.values()) <= 1e-9
    moved = vr.relerr(got['U'], _shared(m, c)['U'])
    print('   U against the shared-weight solve, per instance:', np.array2string(moved, precision=2))
    assert (moved > 1e-2).all()   # an ignored weight argument cannot pass


# ------------------------------------------------------------------------------ 2. the boxes, fp64
@pytest.mark.parametrize('box', ['input', 'state'])
def test_solve_fp64_boxes_match_reference(box):
    spec, c, W, _ = _draw(box)
    ref = _solve_ref(box)
    assert (ref['status'] == 0).all()
    got = _pw(_handle(box), c, W)
    e = _err(got, ref)
    es, _ = _e_shared(box, 'f64')
    print(f'pw17 fp64 {box} box: per-instance error {np.array2string(e, precision=2)}\n'
          f'   shared-weight kernel on a handle with that instance\'s weights {np.array2string(es, precision=2)}')
    assert (got['status'] == 0).all()
    assert (e <= np.maximum(1e-9, 2.0 * es)).all()
    lb, ub = vr.LBU17, vr.UBU17
    assert (got['U'] >= lb - 1e-9).all() and (got['U'] <= ub + 1e-9).all()
    if box == 'state':
        N = spec.N
        n_act = ((ref['X'][:, 1:N] - spec.lbx < 1e-6) | (spec.ubx - ref['X'][:, 1:N] < 1e-6)).sum()
        assert n_act >= 50   # the state box is active (112 rows on this draw)
        assert (got['X'][:, 1:N] >= spec.lbx - 1e-9).all() and (got['X'][:, 1:N] <= spec.ubx + 1e-9).all()


# ------------------------------------------------------------------------------ 3. fp32
@pytest.mark.parametrize('box', ['none', 'input'])
def test_solve_fp32(box):
    spec, c, W, _ = _draw(box)
    ref = _solve_ref(box)
    assert (ref['status'] == 0).all()
    got = _pw(_handle(box, 'f32'), c, W)
    e = _err(got, ref, ('u0',))
    es, sts = _e_shared(box, 'f32', ('u0',))
    print(f'pw17 fp32 {box}: u0 error per instance {np.array2string(e, precision=2)}\n'
          f'   shared-weight kernel on a handle with that instance\'s weights {np.array2string(es, precision=2)}')
    assert (got['status'] == 0).all() and np.array_equal(got['status'], sts)   # every instance converges
    assert (e <= np.maximum(F32_U0[box], 2.0 * es)).all()


# ------------------------------------------------------------------------------ raw calls
def _t(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device='cuda')


def _null():
    return ctypes.c_void_p(0)


def _wptr(w):
    """(pointer, stride) of a weight argument: None, a tensor [B|1, n, n], or an explicit (pointer, stride)."""
    if w is None:
        return _null(), 0
    if isinstance(w, tuple):
        return w
    return ctypes.c_void_p(w.data_ptr()), (0 if w.shape[0] == 1 else w.shape[1] * w.shape[2])


def _raw_solve(m, c, W, B=None, outs=None, x0_sb=17, xref_sb=None, skip=()):
    """mpcb_solve_iterate_pw17 itself.  W: name -> None / tensor / (pointer, stride).  Returns (rc, outputs)."""
    Bc, N = c['ubar'].shape[:2]
    d = {k: _t(c[k], m.dtype) for k in ('x0', 'xbar', 'ubar', 'xref', 'uref')}
    if outs is None:
        outs = dict(u0=torch.full((Bc, 6), 7.0, dtype=m.dtype, device='cuda'),
                    X=torch.full((Bc, N + 1, 17), 7.0, dtype=m.dtype, device='cuda'),
                    U=torch.full((Bc, N, 6), 7.0, dtype=m.dtype, device='cuda'),
                    status=torch.full((Bc,), -77, dtype=torch.int32, device='cuda'))
    P = lambda k: _null() if k in skip else m._ptr(d[k] if k in d else outs[k])   # noqa: E731
    (q, qs), (r, rs), (qn, qns) = (_wptr(W.get(k)) for k in WN)
    rc = m.lib.mpcb_solve_iterate_pw17(m._h, Bc if B is None else B, P('x0'), x0_sb, P('xbar'), P('ubar'), P('xref'),
                                       (N + 1) * 17 if xref_sb is None else xref_sb, P('uref'), N * 6, q, qs, r, rs,
                                       qn, qns, P('u0'), P('X'), P('U'), P('status'), _null())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in outs.items()}


def _raw_vjp(m, c, fixed, W, X=None, U=None, B=None, outs=None, weights=True, skip=()):
    """mpcb_solve_vjp_pw17 itself; every output requested (guard-filled arrays)."""
    Bc, N = c['ubar'].shape[:2]
    d = {k: _t(c[k], m.dtype) for k in ('xbar', 'ubar', 'xref', 'uref', 'gX', 'gU')}
    d['X'], d['U'] = _t(c['xbar'] if X is None else X, m.dtype), _t(c['ubar'] if U is None else U, m.dtype)
    fx = None if fixed is None else _t(fixed, torch.uint8)
    if outs is None:
        shp = dict(gx0=(Bc, 17), gxref=(Bc, N + 1, 17), guref=(Bc, N, 6), gQ=(Bc, 17, 17), gR=(Bc, 6, 6), gQN=(Bc, 17, 17))
        outs = {k: torch.full(s, 7.0, dtype=m.dtype, device='cuda') for k, s in shp.items()}
        outs['status'] = torch.full((Bc,), -77, dtype=torch.int32, device='cuda')
    P = lambda k: _null() if k in skip else m._ptr(d[k] if k in d else outs[k])   # noqa: E731
    (q, qs), (r, rs), (qn, qns) = (_wptr(W.get(k)) for k in WN)
    wo = [P(k) if weights else _null() for k in WKEYS]
    rc = m.lib.mpcb_solve_vjp_pw17(m._h, Bc if B is None else B, P('xbar'), P('ubar'), m._ptr(fx), P('X'), P('U'),
                                   P('xref'), (N + 1) * 17, P('uref'), N * 6, q, qs, r, rs, qn, qns, P('gX'), P('gU'),
                                   P('gx0'), P('gxref'), P('guref'), *wo, P('status'), _null())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in outs.items()}


def _same(a, b, keys=OUT + ('status',)):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ------------------------------------------------------------------------------ 4. weight argument forms
def test_weight_argument_forms():
    spec, c, W, _ = _draw('input')
    B = 6
    m = _handle('input')
    Wd = {k: _t(v) for k, v in W.items()}
    rc, full = _raw_solve(m, c, Wd)
    assert rc == 0 and (full['status'] == 0).all()
    _same(full, _pw(m, c, W))   # the Python layer passes the same contiguous matrices
    # one argument omitted = the handle's matrix, given explicitly
    for k, M in zip(WN, (spec.Q, spec.R, spec.QN)):
        rc, a = _raw_solve(m, c, {**Wd, k: None})
        rc2, b = _raw_solve(m, c, {**Wd, k: _t(np.tile(np.asarray(M)[None], (B, 1, 1)))})
        assert rc == 0 and rc2 == 0
        _same(a, b)
        assert not np.array_equal(a['U'], full['U']), k
    # broadcast (stride 0) against the matrix tiled
    one = {k: _t(v[2:3]) for k, v in W.items()}
    rc, a = _raw_solve(m, c, one)
    rc2, b = _raw_solve(m, c, {k: _t(np.tile(v[2:3], (B, 1, 1))) for k, v in W.items()})
    assert rc == 0 and rc2 == 0 and all(_wptr(v)[1] == 0 for v in one.values())
    _same(a, b)
    assert np.array_equal(a['U'][2], full['U'][2])   # ... and instance 2 is instance 2 of the per-instance run
    # padded strides (the pad is NaN: never read), and bases one element off 16-byte alignment
    padded, off = {}, {}
    for k, v in W.items():
        n2 = v.shape[1] * v.shape[2]
        buf = torch.full((B, n2 + 5), float('nan'), dtype=torch.float64, device='cuda')
        buf[:, :n2] = _t(v).reshape(B, n2)
        padded[k] = (ctypes.c_void_p(buf.data_ptr()), n2 + 5)
        flat = torch.full((B * n2 + 1,), float('nan'), dtype=torch.float64, device='cuda')
        flat[1:] = _t(v).reshape(-1)
        assert flat.data_ptr() % 16 == 0 and (flat.data_ptr() + 8) % 16 == 8
        off[k] = (ctypes.c_void_p(flat.data_ptr() + 8), n2)
        padded['keep_' + k], off['keep_' + k] = buf, flat
    for forms in (padded, off):
        rc, a = _raw_solve(m, c, forms)
        assert rc == 0
        _same(a, full)
    # 2-D diagonals through the Python layer against diag_embed
    rng = np.random.default_rng(3)
    dg = dict(Q=np.diag(spec.Q) * np.exp(rng.normal(0, 0.3, (B, 17))), R=np.diag(spec.R) * np.exp(rng.normal(0, 0.3, (1, 6))),
              QN=np.diag(spec.QN) * np.exp(rng.normal(0, 0.3, (B, 17))))
    a = _pw(m, c, dg)
    b = _pw(m, c, {k: np.stack([np.diag(r) for r in v]) for k, v in dg.items()})
    _same(a, b)
    assert (a['status'] == 0).all() and not np.array_equal(a['U'], full['U'])
    # an unsymmetric 3-D matrix is passed as 0.5 (M + M^T)
    Qa = W['Q'] + np.triu(np.ones((17, 17)), 1) * 1e-3
    _same(_pw(m, c, {**W, 'Q': Qa}), _pw(m, c, {**W, 'Q': 0.5 * (Qa + Qa.transpose(0, 2, 1))}))


# ------------------------------------------------------------------------------ 5. all three NULL
@pytest.mark.parametrize('box', ['none', 'input', 'state'])
def test_all_null_is_solve_iterate_and_leaves_no_trace(box):
    spec, c, W, _ = _draw(box)
    m = _handle(box)
    m.set_timing(True)
    sh = _shared(m, c)
    kern, tim = m.last_kernels(), m.last_timing()
    assert tim['riccati'] > 0
    qs = m.qp_stats(6).cpu().numpy().copy() if box != 'none' else None
    rc, got = _raw_solve(m, c, {})
    assert rc == 0
    _same(got, sh)                                   # the bits of mpcb_solve_iterate
    _pw(m, c, W)                                     # ... then a per-instance call, which iterates differently
    assert m.last_kernels() == kern and 'riccati17q_kernel' in kern['riccati']
    assert m.last_timing() == tim                    # the last timed solve's events, not re-recorded
    if qs is not None:
        assert np.array_equal(m.qp_stats(6).cpu().numpy(), qs)
    # a solve_iterate after the PW calls: the bits of the same call on a fresh handle
    _same(_shared(m, c), _shared(_handle(box), c))
    _same(_shared(m, c), sh)


# ------------------------------------------------------------------------------ 6. chunks and ragged waves
def test_chunked_ragged_run_is_bit_identical(monkeypatch):
    B = 70
    spec, c, W, kw = _draw('input', B)
    one = _pw(_handle('input', B=B), c, W)
    monkeypatch.setenv('MPCB_CHUNK', '64')
    two = _pw(_handle('input', B=B), c, W)   # chunks of 64 and 6: the second ends in a ragged wave
    _same(one, two)
    rows = (63, 64, 69)
    ref = _ref_rows('input', B, rows)
    assert (ref['status'] == 0).all()
    e = _err({k: two[k][list(rows)] for k in OUT}, ref)
    es, _ = _e_shared('input', 'f64', B=B, rows=rows)
    print(f'chunked 64 + 6, instances {rows}: error {np.array2string(e, precision=2)} shared-weight '
          f'{np.array2string(es, precision=2)}')
    assert (two['status'] == 0).all()
    assert (e <= np.maximum(1e-9, 2.0 * es)).all()


# ------------------------------------------------------------------------------ 7. NaN isolation
@pytest.mark.parametrize('box', ['none', 'input'])
@pytest.mark.parametrize('which', WN)
def test_nan_weight_is_isolated_in_the_solve(box, which):
    spec, c, W, _ = _draw(box)
    m = _handle(box)
    ok = _pw(m, c, W)
    Wn = {k: v.copy() for k, v in W.items()}
    Wn[which][1, 2, 2] = np.nan
    got = _pw(m, c, Wn)
    rest = [0, 2, 3, 4, 5]   # 0, 2 and 3 share the wave of instance 1
    assert got['status'][1] == 1 and np.array_equal(got['status'][rest], ok['status'][rest])
    for k in OUT:
        assert np.all(np.isnan(got[k][1])), k
        assert np.array_equal(got[k][rest], ok[k][rest]), k   # bit for bit


@pytest.mark.parametrize('which', WN)
def test_nan_weight_is_isolated_in_the_product(which):
    spec, c, W, _ = _draw('none')
    fixed = vr.random_mask(6, spec.N)
    m = _handle('none')
    Wd = {k: _t(v) for k, v in W.items()}
    rc, ok = _raw_vjp(m, c, fixed, Wd)
    Wn = {k: v.copy() for k, v in W.items()}
    Wn[which][1, 0, 0] = np.inf
    rc2, got = _raw_vjp(m, c, fixed, {k: _t(v) for k, v in Wn.items()})
    assert rc == 0 and rc2 == 0
    rest = [0, 2, 3, 4, 5]
    assert got['status'][1] == 1 and np.all(got['status'][rest] == 0) and np.all(ok['status'] == 0)
    for k in KEYS + WKEYS:
        assert np.all(np.isnan(got[k][1])), k
        assert np.array_equal(got[k][rest], ok[k][rest]), k


# ------------------------------------------------------------------------------ 8. the product and the weight gradients
def _vcheck(got, ref, dtype, tag, keys=KEYS + WKEYS):
    assert np.all(got['status'] == 0), (tag, got['status'])
    err = {k: vr.relerr(got[k].astype(np.float64), ref[k]).max() for k in keys}
    print(f'{tag}: ' + '  '.join(f'{k} {err[k]:.2e}/{VBOUND[dtype]:.0e}' for k in keys))
    for k in keys:
        assert err[k] <= VBOUND[dtype], (tag, k, err[k])


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_product_and_weight_gradients_match_reference(dtype):
    spec, c, W, _ = _draw('none')
    B, N = 6, spec.N
    fixed = vr.random_mask(B, N)
    X = c['xbar'] + 0.1 * np.random.default_rng(6).standard_normal(c['xbar'].shape)
    U = c['ubar'] + 0.1 * np.random.default_rng(7).standard_normal(c['ubar'].shape) * vr.USCALE
    if dtype == 'f32':   # the reference reads the data and the weights as the fp32 handle holds them
        c = {k: _f32(v) for k, v in c.items()}
        W = {k: _f32(v) for k, v in W.items()}
        X, U = _f32(X), _f32(U)
        spec = FullSpec(N=N, cost_scale=float(np.float32(spec.s)))
    ref = pr.pw17_vjp_ref(c['xbar'], c['ubar'], c['p'], fixed, c['gX'], c['gU'], spec, X=X, U=U, xref=c['xref'],
                          uref=c['uref'], **W)
    m = _mpc(N, B, dtype)
    m.set_params(c['p'])
    Wd = {k: _t(v, m.dtype) for k, v in W.items()}
    rc, got = _raw_vjp(m, c, fixed, Wd, X=X, U=U)
    assert rc == 0
    _vcheck(got, ref, dtype, f'pw17 product {dtype} masked')
    for k in WKEYS:
        assert np.array_equal(got[k], np.swapaxes(got[k], 1, 2)), k     # bitwise symmetric
    rc, again = _raw_vjp(m, c, fixed, Wd, X=X, U=U)
    _same(got, again, KEYS + WKEYS + ('status',))                        # two calls, identical bits
    rc, plain = _raw_vjp(m, c, fixed, Wd, X=X, U=U, weights=False)
    _same(got, plain, KEYS)                                              # ... with or without the weight outputs
    assert all(np.all(plain[k] == 7.0) for k in WKEYS)
    # the shared-weight product differs: the weights are read
    sh = m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], fixed=fixed)
    torch.cuda.synchronize()
    assert (vr.relerr(got['gx0'].astype(np.float64), sh['gx0'].cpu().numpy().astype(np.float64)) > 1e-2).all()
    # all weight pointers NULL: the bits of mpcb_solve_vjp17
    rc, nul = _raw_vjp(m, c, fixed, {}, X=X, U=U)
    full = m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], fixed=fixed, X=X, U=U, x_ref=c['xref'],
                               u_ref=c['uref'], weights=True)
    torch.cuda.synchronize()
    assert rc == 0
    _same(nul, {k: v.cpu().numpy() for k, v in full.items() if k != 'fixed'}, KEYS + WKEYS + ('status',))


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_product_end_to_end_with_the_input_box(dtype):
    spec, c, W, _ = _draw('input')
    B, N = 6, spec.N
    tol = 1e-6 if dtype == 'f64' else 1e-3
    m = _handle('input', dtype)
    m.solve_iterate_pw17(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], **W)
    X, U = m.get_state_trajectory(), m.get_input_trajectory()
    assert (m.get_status().cpu().numpy() == 0).all()
    got = m.solve_iterate_vjp_pw17(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], U=U, X=X, x_ref=c['xref'],
                                   u_ref=c['uref'], weights=True, active_tol=tol, **W)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in got.items()}
    o = _solve_ref('input')
    fixed, slack = vr.active_mask(o['U'], spec)
    dev = got['fixed'].astype(bool)
    print(f'pw17 box end to end {dtype}: {fixed.sum()} of {fixed.size} components clamped by the oracle, '
          f'{(dev != fixed).sum()} entries differ on the device at active_tol {tol:g}')
    if dtype == 'f64':
        assert np.array_equal(dev, fixed)   # the oracle's mask, entry for entry
    assert dev.any(axis=(1, 2)).all()
    # the product is checked at what it was given: the mask the layer derived and the solve's own
    # (X, U) (how close those are to the oracle's is the solve's matter, tests 2 and 3)
    cr, Wr = c, W
    if dtype == 'f32':
        cr, Wr = {k: _f32(v) for k, v in c.items()}, {k: _f32(v) for k, v in W.items()}
        spec = FullSpec(N=N, cost_scale=float(np.float32(spec.s)), lbu=vr.LBU17, ubu=vr.UBU17)
    ref = pr.pw17_vjp_ref(cr['xbar'], cr['ubar'], cr['p'], dev, cr['gX'], cr['gU'], spec,
                          X=X.cpu().numpy().astype(np.float64), U=U.cpu().numpy().astype(np.float64),
                          xref=cr['xref'], uref=cr['uref'], **Wr)
    _vcheck(got, ref, dtype, f'pw17 box end to end {dtype}')
    free = m.solve_iterate_vjp_pw17(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], fixed=np.zeros_like(dev), **W)
    torch.cuda.synchronize()
    assert (vr.relerr(free['gx0'].cpu().numpy().astype(np.float64), got['gx0'].astype(np.float64)) > 1e-2).all()


# ------------------------------------------------------------------------------ 9. the torch layer
def test_torch_layer_gradients_equal_the_raw_call():
    from mpc_blaster_amd.autograd import solve_iterate_diff_pw17
    spec, c, W, _ = _draw('input')
    B, N = 6, spec.N
    m = _handle('input')
    before = (m._weights_version, _shared(m, c))
    tt = lambda a, g=True: torch.tensor(a, dtype=torch.float64, device='cuda', requires_grad=g)   # noqa: E731
    gX, gU = _t(c['gX']), _t(c['gU'])
    # 3-D per instance, 2-D [1, 6] diagonals (batch sum), 3-D per instance
    Rd = np.diag(spec.R)[None] * 1.3
    Wt = dict(Q=tt(W['Q']), R=tt(Rd), QN=tt(W['QN']))
    x0, xr, ur = tt(c['x0']), tt(c['xref']), tt(c['uref'][:1])
    u0, X, U = solve_iterate_diff_pw17(m, x0, c['xbar'], c['ubar'], xr, ur, **Wt)
    assert (m.get_status().cpu().numpy() == 0).all()
    ((gX * X).sum() + (gU * U).sum()).backward()
    raw = m.solve_iterate_vjp_pw17(c['xbar'], c['ubar'], gX=gX, gU=gU, U=U.detach(), X=X.detach(), x_ref=c['xref'],
                                   u_ref=c['uref'], weights=True, Q=W['Q'], R=Rd, QN=W['QN'])
    torch.cuda.synchronize()
    assert torch.equal(x0.grad, raw['gx0']) and torch.equal(xr.grad, raw['gxref'])
    assert ur.grad.shape == (1, N, 6) and torch.equal(ur.grad, raw['guref'].sum(dim=0, keepdim=True))
    assert torch.equal(Wt['Q'].grad, raw['gQ']) and torch.equal(Wt['QN'].grad, raw['gQN'])
    assert Wt['R'].grad.shape == (1, 6)
    assert torch.equal(Wt['R'].grad, torch.diagonal(raw['gR'], dim1=1, dim2=2).sum(dim=0, keepdim=True))
    # 2-D [B, 17] diagonals: the diagonal of gQ, instance by instance
    Qd = tt(np.diagonal(W['Q'], axis1=1, axis2=2).copy())
    u0, X, U = solve_iterate_diff_pw17(m, c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], Q=Qd)
    ((gX * X).sum() + (gU * U).sum()).backward()
    raw = m.solve_iterate_vjp_pw17(c['xbar'], c['ubar'], gX=gX, gU=gU, U=U.detach(), X=X.detach(), x_ref=c['xref'],
                                   u_ref=c['uref'], weights=True, Q=Qd.detach())
    assert Qd.grad.shape == (B, 17) and torch.equal(Qd.grad, torch.diagonal(raw['gQ'], dim1=1, dim2=2))
    # a non-OK instance gets zeros: instance 3's R is indefinite
    Rb = np.tile(np.asarray(spec.R)[None], (B, 1, 1))
    Rb[3, 0, 0] = -1e4
    Wt = dict(Q=tt(W['Q']), R=tt(Rb))
    x0 = tt(c['x0'])
    u0, X, U = solve_iterate_diff_pw17(m, x0, c['xbar'], c['ubar'], c['xref'], c['uref'], **Wt)
    st = m.get_status().cpu().numpy()
    assert st[3] != 0 and (np.delete(st, 3) == 0).all()
    (gU * torch.nan_to_num(U)).sum().backward()
    for g in (x0.grad, Wt['Q'].grad, Wt['R'].grad):
        assert torch.all(g[3] == 0) and torch.isfinite(g).all() and all(torch.any(g[b] != 0) for b in (0, 1, 2, 4, 5))
    # the handle's weights are as they were: same version, same bits from the shared-weight solve
    assert m._weights_version == before[0]
    _same(_shared(m, c), before[1])


def test_torch_layer_directional_derivative_in_the_q_diagonals():
    """Unboxed: L = <gX, X> + <gU, U> is smooth in the weights; a central difference along a random
    direction of the Q diagonals against the layer's gradient, 1e-5 relative (the bound of
    test_torch_layer_directional_derivative in tests/test_gpu_vjp17.py)."""
    from mpc_blaster_amd.autograd import solve_iterate_diff_pw17
    spec, c, W, _ = _draw('none')
    B = 6
    m = _handle('none')
    gX, gU = _t(c['gX']), _t(c['gU'])
    q0 = np.diagonal(W['Q'], axis1=1, axis2=2).copy()
    d = q0 * np.random.default_rng(9).standard_normal(q0.shape)   # each entry on its own scale

    def loss(q, grad=False):
        Q = torch.tensor(q, dtype=torch.float64, device='cuda', requires_grad=grad)
        u0, X, U = solve_iterate_diff_pw17(m, c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], Q=Q,
                                           R=W['R'], QN=W['QN'])
        L = (gX * X).sum(dim=(1, 2)) + (gU * U).sum(dim=(1, 2))
        if grad:
            L.sum().backward()
            return Q.grad.cpu().numpy()
        return L.detach().cpu().numpy()

    g = loss(q0, True)
    h = 1e-4
    fd = (loss(q0 + h * d) - loss(q0 - h * d)) / (2.0 * h)
    an = (g * d).sum(axis=1)
    rel = np.abs(fd - an) / np.maximum(np.abs(an), 1e-300)
    print('directional derivative in the Q diagonals, per instance:', np.array2string(rel, precision=2))
    assert (rel <= 1e-5).all()


# ------------------------------------------------------------------------------ 10. closed loop
def test_closed_loop_weights17_is_a_handle_per_instance():
    from mpc_blaster_amd.closed_loop import closed_loop
    B, N, nsim = 4, 6, 3
    spec, c, W, kw = _draw('input')
    c = {k: v[:B] for k, v in c.items()}
    W = {k: v[:B] for k, v in W.items()}
    m = _mpc(N, B, **kw)
    m.set_params(c['p'])
    Xs, Us, st = closed_loop(m, c['x0'], c['xref'], c['uref'], nsim, xbar=c['xbar'], ubar=c['ubar'], weights17=W)
    torch.cuda.synchronize()
    Xs, Us, st = Xs.cpu().numpy(), Us.cpu().numpy(), st.cpu().numpy()
    assert (st == 0).all()
    # the shared-weight run on this handle differs from every instance
    Xh, Uh, _ = closed_loop(m, c['x0'], c['xref'], c['uref'], nsim, xbar=c['xbar'], ubar=c['ubar'])
    assert (vr.relerr(Us, Uh.cpu().numpy()) > 1e-2).all()
    for b in range(B):
        mb = _mpc(N, 1, **kw, **{k: W[k][b] for k in WN})
        mb.set_params(c['p'][b:b + 1])
        r = slice(b, b + 1)
        Xb, Ub, sb = closed_loop(mb, c['x0'][r], c['xref'][r], c['uref'][r], nsim, xbar=c['xbar'][r], ubar=c['ubar'][r])
        torch.cuda.synchronize()
        Xb, Ub = Xb.cpu().numpy(), Ub.cpu().numpy()
        # the reference of this comparison is that run itself (the shared-weight kernel on the same
        # problems), so e_shared is 0 and the rule max(1e-9, 2 e_shared) leaves 1e-9
        e = max(vr.relerr(Xs[r], Xb)[0], vr.relerr(Us[r], Ub)[0])
        print(f'closed loop, instance {b}: against its own handle {e:.2e}')
        assert sb.cpu().numpy()[0] == 0 and e <= 1e-9
        mb.close()


def test_closed_loop_diff_weights17_gradient_and_two_graphs():
    from mpc_blaster_amd.closed_loop import closed_loop_diff
    B, N, nsim = 4, 6, 3
    spec, c, W, _ = _draw('none')
    c = {k: v[:B] for k, v in c.items()}
    W = {k: v[:B] for k, v in W.items()}
    m = _mpc(N, B)
    m.set_params(c['p'])
    xref = _t(c['xref'])
    q0 = np.diagonal(W['Q'], axis1=1, axis2=2).copy()
    col = [2, 0, 4, 14]   # one Q diagonal per instance

    def run(q, grad=False):
        Q = torch.tensor(q, dtype=torch.float64, device='cuda', requires_grad=grad)
        Xs, Us, st = closed_loop_diff(m, c['x0'], c['xref'], c['uref'], nsim, c['xbar'], c['ubar'], warm_start=False,
                                      weights17=dict(Q=Q, R=W['R'], QN=W['QN']))
        assert (st.cpu().numpy() == 0).all()
        L = ((Xs[:, 1:] - xref[:, :nsim]) ** 2).sum(dim=(1, 2))   # summed tracking error, per instance
        return Q, L

    Q1, L1 = run(q0, True)
    Q2, L2 = run(q0 * 1.1, True)       # a second forward graph on the same handle
    L1.sum().backward()                # ... and both backward passes succeed
    L2.sum().backward()
    g = Q1.grad.cpu().numpy()
    assert np.isfinite(g).all() and np.isfinite(Q2.grad.cpu().numpy()).all()
    assert not np.array_equal(g, Q2.grad.cpu().numpy())
    h = 1e-4 * q0[np.arange(B), col]
    qp, qm = q0.copy(), q0.copy()
    qp[np.arange(B), col] += h
    qm[np.arange(B), col] -= h
    fd = (run(qp)[1].detach().cpu().numpy() - run(qm)[1].detach().cpu().numpy()) / (2.0 * h)
    an = g[np.arange(B), col]
    rel = np.abs(fd - an) / np.abs(an)
    print('closed-loop tracking error, d/dQ_ii per instance: central difference '
          f'{np.array2string(fd, precision=6)} layer {np.array2string(an, precision=6)} rel {np.array2string(rel, precision=2)}')
    assert (rel <= 1e-5).all()


# ------------------------------------------------------------------------------ 11. refusals
def test_refusals():
    from mpc_blaster_amd import BatchedMPC, MPCConfig, _lib
    from mpc_blaster_amd.autograd import solve_iterate_diff_pw17
    from mpc_blaster_amd.closed_loop import closed_loop, closed_loop_diff
    spec, c, W, _ = _draw('none')
    B, N = 6, spec.N
    Wd = {k: _t(v) for k, v in W.items()}
    fixed = vr.random_mask(B, N)
    err = lambda m: m.lib.mpcb_last_error().decode()   # noqa: E731
    guard = lambda o, ks: all(np.all(o[k] == 7.0) for k in ks) and np.all(o['status'] == -77)   # noqa: E731

    # a 12/4 handle: both C calls, with a message, and every new Python entry
    m12 = BatchedMPC(MPCConfig(N=N), max_batch=B)
    rc, o = _raw_solve(m12, c, Wd)
    assert rc == E_UNSUPPORTED and 'mpcb_solve_iterate_pw17 covers the 17/6 model' in err(m12) and guard(o, OUT)
    rc, o = _raw_vjp(m12, c, fixed, Wd)
    assert rc == E_UNSUPPORTED and 'mpcb_solve_vjp_pw17 covers the 17/6 model' in err(m12) and guard(o, KEYS + WKEYS)
    z = dict(x0=np.zeros((B, 12)), xbar=np.zeros((B, N + 1, 12)), ubar=np.zeros((B, N, 4)), xref=np.zeros((B, N + 1, 12)),
             uref=np.zeros((B, N, 4)))
    args = (z['x0'], z['xbar'], z['ubar'], z['xref'], z['uref'])
    with pytest.raises(ValueError, match='17/6'):
        m12.solve_iterate_pw17(*args, Q=np.ones((B, 12)))
    with pytest.raises(ValueError, match='17/6'):
        m12.solve_iterate_vjp_pw17(z['xbar'], z['ubar'], gX=z['xbar'])
    with pytest.raises(ValueError, match='17/6'):
        m12.solve_iterate_diff_pw17(*args)
    with pytest.raises(ValueError, match='17/6'):
        solve_iterate_diff_pw17(m12, *args)
    with pytest.raises(ValueError, match='17/6'):
        closed_loop(m12, z['x0'], z['xref'], z['uref'], 2, weights17=dict(Q=np.ones((B, 12))))
    with pytest.raises(ValueError, match='17/6'):
        closed_loop_diff(m12, z['x0'], z['xref'], z['uref'], 2, z['xbar'], z['ubar'], weights17=dict(Q=np.ones((B, 12))))

    # a 17/6 handle: negative strides, missing required arguments, B > max_batch; nothing is written
    m = _handle('none')
    neg = lambda k: {**Wd, k: (ctypes.c_void_p(Wd[k].data_ptr()), -1)}   # noqa: E731
    for k in WN:
        rc, o = _raw_solve(m, c, neg(k))
        assert rc == E_INVALID and 'negative stride' in err(m) and guard(o, OUT), k
        rc, o = _raw_vjp(m, c, fixed, neg(k))
        assert rc == E_INVALID and 'negative stride' in err(m) and guard(o, KEYS + WKEYS), k
    rc, o = _raw_solve(m, c, Wd, xref_sb=-1)
    assert rc == E_INVALID and guard(o, OUT)
    for k in ('x0', 'xbar', 'ubar', 'xref', 'uref', 'u0', 'status'):
        rc, o = _raw_solve(m, c, Wd, skip=(k,))
        assert rc == E_INVALID and guard(o, OUT), k
    for k in ('xbar', 'ubar', 'status', 'X', 'xref'):
        rc, o = _raw_vjp(m, c, fixed, Wd, skip=(k,))
        assert rc == E_INVALID and guard(o, KEYS + WKEYS), k
    rc, o = _raw_vjp(m, c, fixed, Wd, skip=('gX', 'gU'))
    assert rc == E_INVALID and 'no cotangent' in err(m) and guard(o, KEYS + WKEYS)
    rc, o = _raw_solve(m, c, Wd, B=B + 1)
    assert rc == E_INVALID and 'max_batch' in err(m) and guard(o, OUT)
    rc, o = _raw_vjp(m, c, fixed, Wd, B=B + 1)
    assert rc == E_INVALID and guard(o, KEYS + WKEYS)
    # the Python layer's own checks
    with pytest.raises(ValueError, match='expected'):
        m.solve_iterate_pw17(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], Q=np.ones((B, 12)))
    with pytest.raises(ValueError, match='batch'):
        m.solve_iterate_pw17(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], Q=np.ones((B - 1, 17)))
    with pytest.raises(ValueError, match='unknown keys'):
        closed_loop(m, c['x0'], c['xref'], c['uref'], 2, weights17=dict(P=W['Q']))
    with pytest.raises(ValueError, match='unknown keys'):
        closed_loop_diff(m, c['x0'], c['xref'], c['uref'], 2, c['xbar'], c['ubar'], weights17=dict(P=W['Q']))
    with pytest.raises(ValueError, match='feedback'):
        closed_loop(m, c['x0'], c['xref'], c['uref'], 2, weights17=dict(Q=W['Q']), feedback=True)
    with pytest.raises(ValueError, match='diagnostics'):
        closed_loop(m, c['x0'], c['xref'], c['uref'], 2, weights17=dict(Q=W['Q']), diagnostics=True)

    # the state box: refused in the product and in the layer (the solve serves it: test 2)
    _, cs, Ws, _ = _draw('state')
    ms = _handle('state')
    cs = dict(cs, gX=np.ones_like(cs['xbar']), gU=np.ones_like(cs['ubar']))
    rc, o = _raw_vjp(ms, cs, None, {k: _t(v) for k, v in Ws.items()})
    assert rc == E_UNSUPPORTED and 'state box' in err(ms) and guard(o, KEYS + WKEYS)
    with pytest.raises(ValueError, match='state box'):
        ms.solve_iterate_diff_pw17(cs['x0'], cs['xbar'], cs['ubar'], cs['xref'], cs['uref'], Q=Ws['Q'])
    with pytest.raises(ValueError, match='state box'):
        closed_loop_diff(ms, cs['x0'], cs['xref'], cs['uref'], 2, cs['xbar'], cs['ubar'], weights17=dict(Q=Ws['Q']))
    # f32 with the input box and no active_tol, as solve_iterate_diff
    _, cu, Wu, _ = _draw('input')
    with pytest.raises(ValueError, match='active_tol'):
        _handle('input', 'f32').solve_iterate_diff_pw17(cu['x0'], cu['xbar'], cu['ubar'], cu['xref'], cu['uref'], Q=Wu['Q'])

    # the existing refusals of the 12/4 keywords on a 17/6 handle are still raised
    with pytest.raises(ValueError, match='12/4'):
        m.solve_iterate(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], Q=W['Q'])
    with pytest.raises(ValueError, match='12/4'):
        m.solve_iterate_diff(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], Q=torch.ones(B, 17), per_instance_weights=True)
    with pytest.raises(ValueError, match='takes no weights'):
        closed_loop_diff(m, c['x0'], c['xref'], c['uref'], 2, c['xbar'], c['ubar'], weights=dict(Q=W['Q']))
    rc = m.lib.mpcb_solve_iterate_pw(m._h, B, *([_null(), 0] * 1), _null(), _null(), _null(), 0, _null(), 0, _null(), 0,
                                     _null(), 0, _null(), 0, _null(), 0, _null(), _null(), _null(), _null(), _null())
    assert rc == E_UNSUPPORTED and err(m) == 'per-instance weights cover the 12/4 model only'
