"""The fused fp64 rollout + Riccati kernel (row_riccati_kernel, the c2 path) at the shapes where its
row prologue can go wrong: the lane constants now come from a table filled at create time
(Weights::rowt) and every row of the wave stages its own instance's inputs into LDS with 16-byte
copies from one base pointer.

- horizons 1, 2, 3, 20, and 33 and 65: at fp64 a row stages N * 4 / 2 vectors, eight per lane and
  pass, so 33 leaves a partly filled pass and 65 (130 vectors) is the first horizon that takes the
  second pass of the staging loop;
- batches 1, 3, 5 and 65: a lone instance, ragged quads (the spare rows restage the last
  instance) and a second workgroup;
- u_ref per instance (every instance its own record, so a row that staged a neighbour's record
  shows) and broadcast with stride 0; rollout and iterate mode; the reference's diagonal inertia
  and a general one; wind on and off (the wind's share of f's constant term is still built in the
  kernel, on top of the table's gravity slot);
- the fused launch against the two-launch build of the same bodies, bit for bit;
- the launches are the two kernels the c2 plan names.

Tolerance: 1e-9 relative (relerr: per instance, against max(|reference|, 1)) on u0 / X / U against
the NumPy oracle, the bound tests/test_gpu_c2_trim.py uses for the same path and oracle.
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

BMAX = 65
TOL = 1e-9
FUSED = {'rollout': 'mpcb::row_riccati_kernel<false, true>', 'iterate': 'mpcb::row_riccati_kernel<true, true>'}
FORWARD = 'mpcb::fwd_rm_kernel<double, false>'


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


def _general_j():
    J = np.diag([0.50781, 0.47314, 0.72975])
    J[0, 1] = J[1, 0] = 0.01
    return J


@functools.lru_cache(maxsize=None)
def _inputs(N, B):
    """c2's inputs with a u_ref record of its own per instance and stage, an iterate and a wind."""
    inp = make_inputs('c2', ids=np.arange(B, dtype=np.uint64), N=N)
    rng = np.random.default_rng(33)
    inp['uref'] = inp['uref'] + rng.uniform(-1.0, 1.0, size=(B, N, 4))
    inp['xbar'] = inp['xref'] + rng.normal(scale=0.05, size=(B, N + 1, 12))
    inp['ubar'] = inp['uref'] + rng.normal(scale=1.0, size=(B, N, 4))
    inp['wind'] = rng.uniform(-5.0, 5.0, size=(B, 3))
    return inp


def _args(N, B, nref, bcast, wind):
    inp = _inputs(N, nref)
    a = {k: inp[k][:B] for k in ('x0', 'xref', 'uref', 'xbar', 'ubar')}
    if bcast:
        a['uref'] = inp['uref'][:1]
    a['wind'] = inp['wind'][:B] if wind else None
    return a


@functools.lru_cache(maxsize=None)
def _oracle(N, nref, mode, general_j, bcast, wind):
    """One reference per case at the largest batch of its tests; smaller batches are its leading
    instances (the inputs are drawn per instance id)."""
    a = _args(N, nref, nref, bcast, wind)
    spec = OcpSpec(N=N, **({'params': Params(J=_general_j())} if general_j else {}))
    uref = np.broadcast_to(a['uref'], (nref, N, 4))
    if mode == 'iterate':
        return mpc_solve(a['x0'], a['xref'], uref, spec, wind=a['wind'], mode='iterate', xbar=a['xbar'], ubar=a['ubar'])
    return mpc_solve(a['x0'], a['xref'], uref, spec, wind=a['wind'])


def _solve(m, a, mode):
    if mode == 'iterate':
        m.solve_iterate(a['x0'], a['xbar'], a['ubar'], a['xref'], a['uref'], wind=a['wind'])
    else:
        m.solve(a['x0'], a['xref'], a['uref'], wind=a['wind'])
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for t in (m.get_control(), m.get_state_trajectory(),
                                             m.get_input_trajectory(), m.get_status())]


def _check(N, B, mode, nref, general_j=False, bcast=False, wind=False, fused=True):
    m = _mpc(N, B, **({'J': _general_j()} if general_j else {}))
    u0, X, U, status = _solve(m, _args(N, B, nref, bcast, wind), mode)
    if fused:
        kernel = FUSED[mode].replace('true>', 'false>') if general_j else FUSED[mode]
        assert m.last_kernels()['riccati'] == kernel
    else:   # the same row body as a launch of its own (mpcb_rollout.hip)
        assert 'nominal_row_kernel<double' in m.last_kernels()['nominal']
    o = _oracle(N, nref, mode, general_j, bcast, wind)
    e = [relerr(u0, o['u0'][:B]).max(), relerr(X, o['X'][:B]).max(), relerr(U, o['U'][:B]).max()]
    print(f'N={N} B={B} {mode} J={"general" if general_j else "diagonal"} bcast={bcast} wind={wind}: '
          f'max rel err u0 {e[0]:.2e} X {e[1]:.2e} U {e[2]:.2e}')
    assert (status == 0).all()
    assert max(e) < TOL


@pytest.mark.parametrize('mode', ['rollout', 'iterate'])
@pytest.mark.parametrize('B', [1, 3, 5, 65])
@pytest.mark.parametrize('N', [1, 2, 3, 20])
def test_per_instance_uref_matches_oracle(N, B, mode):
    _check(N, B, mode, BMAX)


@pytest.mark.parametrize('mode', ['rollout', 'iterate'])
@pytest.mark.parametrize('B', [3, 65])
@pytest.mark.parametrize('N', [1, 20])
def test_broadcast_uref_matches_oracle(N, B, mode):
    _check(N, B, mode, BMAX, bcast=True)


@pytest.mark.parametrize('mode', ['rollout', 'iterate'])
@pytest.mark.parametrize('wind', [False, True])
@pytest.mark.parametrize('general_j', [False, True])
def test_inertia_and_wind_match_oracle(general_j, wind, mode):
    _check(3, 5, mode, 5, general_j=general_j, wind=wind)


@pytest.mark.parametrize('mode', ['rollout', 'iterate'])
@pytest.mark.parametrize('N', [33, 65])
def test_staging_partial_and_second_pass_match_oracle(N, mode):
    """Past N = 32 the two bodies' LDS no longer fits one wave per SIMD and the rollout runs as
    its own launch: the same row_body and staging code."""
    _check(N, 5, mode, 5, fused=False)


@pytest.mark.parametrize('mode', ['rollout', 'iterate'])
def test_fused_kernel_equals_two_launches(mode):
    """MPCB_FUSE_P12=0 runs the same two bodies as two launches: the same bits, wind included."""
    res = []
    for fuse in ('1', '0'):
        m = _mpc(3, 5, env={'MPCB_FUSE_P12': fuse})
        res.append(_solve(m, _args(3, 5, 5, False, True), mode))
        if fuse == '1':
            assert m.last_kernels()['riccati'] == FUSED[mode]
        else:
            assert 'row_riccati' not in m.last_kernels()['riccati']
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_c2_launches_are_the_planned_pair():
    m = _mpc(20, BMAX)
    _solve(m, _args(20, BMAX, BMAX, False, False), 'rollout')
    last, plan = m.last_kernels(), m.plan_kernels(BMAX)
    print(last)
    assert last == plan
    assert last == {'riccati': FUSED['rollout'], 'forward': FORWARD}
