"""The 12/4 input box at every ``max_as_iter``: the cap decides which kernels solve an instance
(the active set alone, the active set then the interior point, the interior point from the start;
in fp32 the refinement kernel after either), never what comes out.

The contract (INTEGRATION.md "Rules of the ABI"): an instance that reaches
min(max_as_iter, 48) passes does not end as MAXITER, it goes on in the interior point
(as_ipm_kernel) and in fp32 through the refinement kernel (as_ref_kernel_f32); max_as_iter = 1 is
the interior point from the start.

The draw is the hard-box draw of tests/test_gpu_edges.py (sine references, +-5 N wind, B = 192,
N = 18, box 0 <= u <= 65), in rollout mode and in that file's iterate mode.  The oracle
(oracle.ocp.mpc_solve at the same cap) gives, for this draw, all OK at every cap and

  hand-overs, rollout, cap 1 2 3 5 9 10 11 20 47 48:  192 188 181 121 63 57 53 40 26 26
  hand-overs, iterate, cap 1 / 48:                    192 / 43
  converged by the active set in >= 10 passes, cap 48: 37 (rollout, up to 41 passes),
                                                       26 (iterate, up to 43)
  fp32_sensitivity > 1e-5 on fp32-rounded inputs:      17 of 192 rollout, 18 iterate

so that most caps in 11..48 have an instance that converges on its last allowed pass (the fp32
refinement list takes converged instances from AS_REF_PASSES = 10 passes on).  The oracle's U
differs by at most 3.9e-9 between caps, so the cap-48 solve is the reference of every fp32 cap.

Before the refinement kernel had a pass budget of its own (mpcb_as.h AS_REF_BUDGET) it applied the
active set's cap to its refined passes, counted from the listed pass count, and wrote MAXITER over
an instance that an earlier kernel had finished as OK: the fp32 sweep below failed at the caps
named in its docstring.  The fp64 statistics agree with the oracle's counts exactly, hand-overs
included.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle.ocp import AS_IPM_AFTER, OcpSpec, fp32_sensitivity, mpc_solve

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

N, B = 18, 192
LBU, UBU = 0.0, 65.0
MODES = ('rollout', 'iterate')
CAPS64 = (1, 2, 3, 5, 9, 10, 11, 20, 47, 48, 49, 200)
# the oracle's hand-overs on this draw (module docstring); the cap is clamped to 48
HANDED = {'rollout': {1: 192, 2: 188, 3: 181, 5: 121, 9: 63, 10: 57, 11: 53, 20: 40, 47: 26, 48: 26, 49: 26,
                      200: 26},
          'iterate': {1: 192, 48: 43, 49: 43, 200: 43}}
# fp32: every cap the clamp leaves distinct, and the default
CAPS32 = tuple(range(1, AS_IPM_AFTER + 1)) + (200,)
CAP_GROUPS = tuple(CAPS32[i:i + 8] for i in range(0, 48, 8))
CAP_GROUPS = CAP_GROUPS[:-1] + (CAP_GROUPS[-1] + (200,),)
ILL_MAX = 18          # instances fp32 data cannot pin (fp32_sensitivity > 1e-5), chosen by the oracle alone
MPCB_E_UNSUPPORTED = -4
AS_REF_PASSES = 10    # mpcb_kernels.h: converged instances are listed for the refinement from here on


def relerr(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(a.shape[0], -1)
    b = np.asarray(b, dtype=np.float64).reshape(b.shape[0], -1)
    return np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1.0)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _inputs(mode, dtype):
    from test_oracle_ocp import hard_box_inputs
    inp = hard_box_inputs(B, N, 11)
    cast = (lambda a: a.astype(np.float32).astype(np.float64)) if dtype == 'f32' else (lambda a: a)
    i = {k: cast(inp[k]) for k in ('x0', 'xref', 'uref', 'wind')}
    if mode == 'iterate':
        rng = np.random.default_rng(3)
        i['xbar'] = cast(inp['xref'] + rng.normal(scale=0.05, size=(B, N + 1, 12)))
        i['ubar'] = cast(inp['uref'] + rng.normal(scale=1.0, size=(B, N, 4)))
    return _frozen(i)


def _spec(cap):
    return OcpSpec(N=N, lbu=np.full(4, LBU), ubu=np.full(4, UBU), max_as_iter=cap)


@functools.lru_cache(maxsize=None)
def _oracle(mode, cap, dtype):
    i = _inputs(mode, dtype)
    kw = dict(mode='iterate', xbar=i['xbar'], ubar=i['ubar']) if mode == 'iterate' else {}
    return _frozen(mpc_solve(i['x0'], i['xref'], i['uref'], _spec(cap), wind=i['wind'], return_lin=True, **kw))


@functools.lru_cache(maxsize=None)
def _reference32(mode):
    """The fp32 sweep's reference: the cap-48 oracle on fp32-rounded inputs, the instances fp32
    data can pin, and the QP's optimal objective."""
    from test_gpu_fuzz import qp_objective
    i, o, spec = _inputs(mode, 'f32'), _oracle(mode, AS_IPM_AFTER, 'f32'), _spec(AS_IPM_AFTER)
    sens = fp32_sensitivity(o, i['x0'], i['xref'], i['uref'], spec)
    jopt = np.abs(qp_objective(o, o['U'], i['x0'], i['xref'], i['uref'], spec))
    return o, sens <= 1e-5, jopt


def _solve(mode, cap, dtype):
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    m = BatchedMPC(MPCConfig(N=N, dtype=dtype, lbu=np.full(4, LBU), ubu=np.full(4, UBU), max_as_iter=cap),
                   max_batch=B)
    i = _inputs(mode, dtype)
    if mode == 'iterate':
        m.solve_iterate(i['x0'], i['xbar'], i['ubar'], i['xref'], i['uref'], wind=i['wind'])
    else:
        m.solve(i['x0'], i['xref'], i['uref'], wind=i['wind'])
    torch.cuda.synchronize()
    out = [t.cpu().numpy().copy() for t in (m.get_control(), m.get_state_trajectory(), m.get_input_trajectory(),
                                            m.get_status())]
    return m, out


def _ref_list(m):
    """[instances listed, the refinement kernel's counter] of the handle's last fp32 box chunk."""
    rl = (ctypes.c_int32 * 2)()
    rc = m.lib.mpcb_debug_ref_list(m._h, rl)
    return rc, int(rl[0]), int(rl[1])


# ------------------------------------------------------------------------------ fp64
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('cap', CAPS64)
def test_fp64_cap_matches_oracle_at_the_same_cap(cap, mode):
    """fp64, the device against the oracle at the same cap: same statuses (all OK), u0 / X / U
    within 1e-9 normwise, U inside the box to 1e-7; and mpcb_qp_stats' first column (forward passes
    plus interior-point iterations) against the oracle's count: equal where the active set
    converged (the same rule on outputs that agree to 1e-9), within +-2 on a hand-over (the 17/6
    test allows +-1 for one interior point; this path also crosses the active-set / interior-point
    seam).  Non-vacuity on the oracle alone: its hand-overs are the module docstring's, and caps
    48, 49 and 200 give identical oracle output (the clamp)."""
    o = _oracle(mode, cap, 'f64')
    fb = o['fallback']
    print(f'f64 {mode} cap {cap}: oracle hands over {int(fb.sum())}, passes of the others up to '
          f'{int(o["iters"][~fb].max(initial=0))}')
    if cap in HANDED[mode]:
        assert fb.sum() == HANDED[mode][cap]
    if cap > AS_IPM_AFTER:
        o48 = _oracle(mode, AS_IPM_AFTER, 'f64')
        for k in ('u0', 'X', 'U', 'status', 'iters', 'fallback'):
            assert np.array_equal(o[k], o48[k]), k
    m, (u0, X, U, st) = _solve(mode, cap, 'f64')
    e = np.maximum(np.maximum(relerr(u0, o['u0']), relerr(X, o['X'])), relerr(U, o['U']))
    print(f'  status {np.bincount(st, minlength=5).tolist()}, max rel err {e.max():.2e}')
    assert (o['status'] == 0).all()
    assert (st == o['status']).all()
    assert e.max() < 1e-9
    assert (U >= LBU - 1e-7).all() and (U <= UBU + 1e-7).all()
    # the statistics
    it = m.qp_stats(B).cpu().numpy()[:, 0].astype(np.int64)
    d = it - o['iters']
    print(f'  qp_stats[:, 0] - oracle iters: converged by the active set {int(np.abs(d[~fb]).max(initial=0))} '
          f'(of {int((~fb).sum())}), handed over min {int(d[fb].min(initial=0))} max {int(d[fb].max(initial=0))}')
    if (d[~fb] != 0).any():
        w = np.nonzero(~fb & (d != 0))[0][:8]
        print(f'  differ: instances {w.tolist()} device {it[w].tolist()} oracle {o["iters"][w].tolist()}')
    assert (d[~fb] == 0).all()
    assert (np.abs(d[fb]) <= 2).all()


# ------------------------------------------------------------------------------ fp32
def _check32(mode, cap, out):
    """The fp32 acceptance of one cap against the cap-48 oracle; returns (problems, worst error of
    the instances fp32 data can pin, worst objective gap)."""
    from test_gpu_fuzz import qp_objective
    u0, X, U, st = out
    i = _inputs(mode, 'f32')
    o, pin, jopt = _reference32(mode)
    e = np.maximum(np.maximum(relerr(u0, o['u0']), relerr(X, o['X'])), relerr(U, o['U']))
    gap = qp_objective(o, U, i['x0'], i['xref'], i['uref'], _spec(AS_IPM_AFTER)) / jopt - 1.0
    bad = []
    if not (st == 0).all():
        w = np.nonzero(st != 0)[0]
        bad.append(f'status histogram {np.bincount(st, minlength=5).tolist()}, not OK: instances {w[:12].tolist()} '
                   f'(oracle passes {o["iters"][w[:12]].tolist()}, handed over {o["fallback"][w[:12]].tolist()})')
    if not ((U >= LBU - 2e-4).all() and (U <= UBU + 2e-4).all()):
        bad.append(f'U outside the box: min {U.min():.6g} max {U.max():.6g}')
    over = pin & (e >= 5e-5)
    if over.any():
        w = np.nonzero(over)[0]
        w = w[np.argsort(-e[w])][:8]
        bad.append(f'{int(over.sum())} instances beyond 5e-5: {w.tolist()} err {[f"{x:.2e}" for x in e[w]]} '
                   f'status {st[w].tolist()}')
    if not (gap < 1e-5).all():
        w = np.nonzero(~(gap < 1e-5))[0]
        w = w[np.argsort(-gap[w])][:8]
        bad.append(f'objective gap: {w.tolist()} gap {[f"{x:.2e}" for x in gap[w]]} status {st[w].tolist()}')
    return bad, float(e[pin].max()), float(gap.max())


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('caps', CAP_GROUPS, ids=lambda c: f'{c[0]}-{c[-1]}')
def test_fp32_every_cap_ends_ok_and_matches_oracle(caps, mode):
    """fp32, one handle per cap, every cap 1..48 and 200: every status OK (the contract), U inside
    the box to 2e-4, every instance that fp32 data can pin (fp32_sensitivity <= 1e-5 on the cap-48
    oracle, at most 18 of 192 left out) within 5e-5 normwise on u0 / X / U, every instance within
    1e-5 of the QP's optimal objective.

    With the refinement kernel under the active set's cap this failed with MAXITER written over
    instances that an earlier kernel had finished as OK: rollout caps 1 and 2 (status histogram
    [189, 0, 3, 0, 0]: hand-overs whose one refined pass changed the set, up to 2.6e-4 off), iterate
    caps 1 and 2 ([190, 0, 2, 0, 0]), rollout caps 35 and 36 ([191, 0, 1, 0, 0]: an instance that
    converges on pass 35, 4.5e-4 off).  Every other cap passed."""
    o, pin, _ = _reference32(mode)
    assert (o['status'] == 0).all()
    assert (~pin).sum() <= ILL_MAX
    failures = {}
    for cap in caps:
        bad, ew, gw = _check32(mode, cap, _solve(mode, cap, 'f32')[1])
        print(f'f32 {mode} cap {cap}: max rel err of the {int(pin.sum())} pinned {ew:.2e}, objective gap max {gw:.2e}'
              + ''.join(f'\n    FAIL {b}' for b in bad))
        if bad:
            failures[cap] = bad
    assert not failures, f'{mode}: caps {sorted(failures)} fail: {failures}'


@pytest.mark.parametrize('mode', MODES)
def test_fp32_refinement_ran_on_every_ok_handover(mode):
    """Every fp32 hand-over that the interior point finishes as OK is listed for the refinement
    kernel (mpcb_asipm.h): after the cap-1 solve (all 192 handed over) and the cap-48 solve the
    list holds at least the oracle's hand-overs whose device status is OK."""
    from mpc_blaster_amd import load_library
    if not hasattr(load_library(), 'mpcb_debug_ref_list'):
        pytest.skip('the library has no mpcb_debug_ref_list')
    for cap in (1, AS_IPM_AFTER):
        fb = _oracle(mode, cap, 'f32')['fallback']
        m, (_, _, _, st) = _solve(mode, cap, 'f32')
        rc, listed, walked = _ref_list(m)
        want = int((fb & (st == 0)).sum())
        print(f'f32 {mode} cap {cap}: {listed} listed (counter {walked}); {int(fb.sum())} oracle hand-overs, {want} OK')
        assert rc == 0
        assert fb.sum() == (B if cap == 1 else HANDED[mode][cap])
        assert want == fb.sum()
        assert want <= listed <= B


def test_debug_ref_list_is_refused_without_a_refinement_list():
    """Only a 12/4 fp32 input-box handle has a refinement list: a 12/4 fp64 box handle and a 17/6
    box handle never initialise that region, so the diagnostic refuses them."""
    from mpc_blaster_amd import BatchedMPC, MPCConfig, load_library
    from test_gpu_full17 import LBU17, UBU17
    if not hasattr(load_library(), 'mpcb_debug_ref_list'):
        pytest.skip('the library has no mpcb_debug_ref_list')
    m64, _ = _solve('rollout', AS_IPM_AFTER, 'f64')
    m17 = BatchedMPC(MPCConfig.full(N=6, lbu=LBU17, ubu=UBU17), max_batch=8)
    m17f = BatchedMPC(MPCConfig.full(N=6, dtype='f32', lbu=LBU17, ubu=UBU17), max_batch=8)
    for m in (m64, m17, m17f):
        assert _ref_list(m)[0] == MPCB_E_UNSUPPORTED
    assert b'refinement' in m64.lib.mpcb_last_error()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('cap', [5, 11, 20])
def test_fp32_cap_leaves_early_converged_instances_bit_identical(cap, mode):
    """An instance that the oracle hands over neither at cap m nor at cap 48 and that converges in
    fewer than min(m, 10) passes meets the cap in no kernel: its fp32 outputs at cap m are those
    at cap 48 bit for bit."""
    om, o48 = _oracle(mode, cap, 'f32'), _oracle(mode, AS_IPM_AFTER, 'f32')
    sel = ~om['fallback'] & ~o48['fallback'] & (o48['iters'] < min(cap, AS_REF_PASSES))
    assert np.array_equal(om['iters'][sel], o48['iters'][sel])
    print(f'f32 {mode} cap {cap}: {int(sel.sum())} instances converge in fewer than {min(cap, AS_REF_PASSES)} passes')
    assert sel.sum() >= 30   # (the oracle: 30 / 34 at cap 5, 129 / 123 at caps 11 and 20, rollout / iterate)
    _, got = _solve(mode, cap, 'f32')
    _, ref = _solve(mode, AS_IPM_AFTER, 'f32')
    for name, a, b in zip(('u0', 'X', 'U', 'status'), got, ref):
        d = np.nonzero((a[sel] != b[sel]).reshape(int(sel.sum()), -1).any(axis=1))[0]
        if len(d):
            w = np.nonzero(sel)[0][d[:8]]
            print(f'  {name} differs on {len(d)} instances, e.g. {w.tolist()} (oracle passes {o48["iters"][w].tolist()})')
        assert not len(d), name
