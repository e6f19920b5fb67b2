"""The fused fp64 rollout + Riccati kernel (row_riccati_kernel, the c2 path) at the shapes where
its stage hand-over can go wrong: horizons 1, 2, 3 (no stage to load ahead, then the two parities)
and 20, batches with partial quads and a partial last wave, dense weights (the default ones are
diagonal and would hide a transposed or mis-strided weight table), a general inertia, and the
fused launch against the two-launch build of the same bodies.

Tolerance: 1e-9 relative (relerr: per instance, against max(|reference|, 1)) on u0 / X / U, the
bound the other fp64 parity tests of this path use against the same oracle.
"""
import functools
import os

import numpy as np
import pytest

from oracle.inputs import make_inputs
from oracle.model import Params
from oracle.ocp import OcpSpec, mpc_solve

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

BMAX = 67
TOL = 1e-9
FUSED = {'rollout': 'mpcb::row_riccati_kernel<false, true>', 'iterate': 'mpcb::row_riccati_kernel<true, true>'}


def _mpc(N, B, env=None, **kw):
    """fp64 handle on the split path (forced as tests/test_gpu_parity.py does)."""
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    env = dict({'MPCB_SPLIT_MIN_BATCH': '1'}, **(env or {}))
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return BatchedMPC(MPCConfig(N=N, dtype='f64', **kw), max_batch=B)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def relerr(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(a.shape[0], -1)
    b = np.asarray(b, dtype=np.float64).reshape(b.shape[0], -1)
    return np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1.0)


def _spd(rng, n, scale):
    m = rng.normal(size=(n, n))
    return scale * (m @ m.T / n + np.eye(n))


@functools.lru_cache(maxsize=None)
def _weights(kind):
    if kind == 'default':
        return {}
    rng = np.random.default_rng(7)
    return {'Q': _spd(rng, 12, 5.0), 'R': _spd(rng, 4, 0.1), 'QN': _spd(rng, 12, 50.0)}


@functools.lru_cache(maxsize=None)
def _inputs(N, B):
    inp = make_inputs('c2', ids=np.arange(B, dtype=np.uint64), N=N)
    rng = np.random.default_rng(21)
    inp['xbar'] = inp['xref'] + rng.normal(scale=0.05, size=(B, N + 1, 12))
    inp['ubar'] = inp['uref'] + rng.normal(scale=1.0, size=(B, N, 4))
    return inp


@functools.lru_cache(maxsize=None)
def _oracle(N, B, mode, kind, general_j=False):
    """One reference per (horizon, mode, weights) at the largest batch of its tests; smaller batches
    are its leading instances (the inputs are drawn per instance id)."""
    inp = _inputs(N, B)
    kw = dict(_weights(kind))
    if general_j:
        kw['params'] = Params(J=_general_j())
    spec = OcpSpec(N=N, **kw)
    if mode == 'iterate':
        return mpc_solve(inp['x0'], inp['xref'], inp['uref'], spec, mode='iterate', xbar=inp['xbar'], ubar=inp['ubar'])
    return mpc_solve(inp['x0'], inp['xref'], inp['uref'], spec)


def _general_j():
    J = np.diag([0.50781, 0.47314, 0.72975])
    J[0, 1] = J[1, 0] = 0.01
    return J


def _solve(m, inp, B, mode):
    a = {k: v[:B] for k, v in inp.items() if isinstance(v, np.ndarray) and v.shape[:1] == inp['x0'].shape[:1]}
    if mode == 'iterate':
        m.solve_iterate(a['x0'], a['xbar'], a['ubar'], a['xref'], a['uref'])
    else:
        m.solve(a['x0'], a['xref'], a['uref'])
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for t in (m.get_control(), m.get_state_trajectory(),
                                             m.get_input_trajectory(), m.get_status())]


def _check(N, B, mode, kind, nref, kernel, **cfg):
    m = _mpc(N, B, **dict(_weights(kind), **cfg))
    u0, X, U, status = _solve(m, _inputs(N, nref), B, mode)
    assert m.last_kernels()['riccati'] == kernel
    o = _oracle(N, nref, mode, kind, 'J' in cfg)
    e = [relerr(u0, o['u0'][:B]).max(), relerr(X, o['X'][:B]).max(), relerr(U, o['U'][:B]).max()]
    print(f'N={N} B={B} {mode} {kind}: max rel err u0 {e[0]:.2e} X {e[1]:.2e} U {e[2]:.2e}')
    assert (status == 0).all()
    assert max(e) < TOL


@pytest.mark.parametrize('mode', ['rollout', 'iterate'])
@pytest.mark.parametrize('B', [1, 3, 5, 67])
@pytest.mark.parametrize('N', [1, 2, 3, 20])
def test_fused_kernel_matches_oracle(N, B, mode):
    _check(N, B, mode, 'default', BMAX, FUSED[mode])


@pytest.mark.parametrize('mode', ['rollout', 'iterate'])
@pytest.mark.parametrize('N', [1, 2, 3])
def test_fused_kernel_dense_weights_match_oracle(N, mode):
    _check(N, 5, mode, 'dense', 5, FUSED[mode])


@pytest.mark.parametrize('mode', ['rollout', 'iterate'])
def test_fused_kernel_general_inertia_matches_oracle(mode):
    kernel = 'mpcb::row_riccati_kernel<%s, false>' % ('true' if mode == 'iterate' else 'false')
    _check(3, 5, mode, 'default', 5, kernel, J=_general_j())


@pytest.mark.parametrize('mode', ['rollout', 'iterate'])
@pytest.mark.parametrize('N', [1, 2, 3])
def test_fused_kernel_equals_two_launches(N, mode):
    """MPCB_FUSE_P12=0 runs the same two bodies as two launches: the same bits."""
    res = []
    for fuse in ('1', '0'):
        m = _mpc(N, 5, env={'MPCB_FUSE_P12': fuse})
        res.append(_solve(m, _inputs(N, 5), 5, mode))
        if fuse == '1':
            assert m.last_kernels()['riccati'] == FUSED[mode]
        else:
            assert 'row_riccati' not in m.last_kernels()['riccati']
    for a, b in zip(*res):
        assert np.array_equal(a, b)
