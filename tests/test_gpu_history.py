"""A handle's results do not depend on its call history.

The rest of the GPU suite creates a handle, calls one entry point at one batch size and compares.
``closed_loop``, ``closed_loop_diff`` and a training loop keep one handle alive and send it solves,
gains, products, plant steps and setters in some order at changing batch sizes.  Here fixed call
programmes (tests/history_calls.py: PROGRAMME, SCHEDULE, the kinds) run on one handle, and every
output of every call must equal, BIT FOR BIT, the same call on a fresh handle: same config, same
max_batch, same environment switches at creation, no other call made (``history_calls.fresh``).
Where setters reconfigured the handle under test, the fresh handle is created with the final values
in its config (``set_params`` has no config counterpart and is applied to the fresh handle too).

No output of any entry point was found that is not reproducible run to run on fresh handles (no
floating-point atomic reaches an output; the histogram's integer atomics commute), so nothing is
exempt from bit equality.

Handle state (struct mpcb_handle, mpcb_capi.hip) -> the test that exercises it
    shared chunk workspace (solve, solve_iterate, linearize, evaluate; never cleared): a call at
      B = 6 or 3 after one at 79, 70 or 65, ghost groups in the last wave, the second chunk of the
      MPCB_CHUNK=64 kinds at 70 and 65                       test_programme (both orders)
    lazily allocated vjp_scratch, gains_scratch, pw_scratch, vjp17_scratch (the last shared by
      mpcb_solve_vjp17 and the 17/6 mpcb_solve_gains): first call at B = 1 in one order, at B = 79 in
      the other                                               test_programme, asserted from the table
                                                              by test_first_calls_of_the_lazy_workspaces
    box bookkeeping (active-set work counter, interior-point hand-over list, fp32 refinement list,
      qp_stats_rows, u_scratch of the fp32 box without U): solve / solve(want_traj=False) adjacent in
      both orders, other entry points between, qp_stats re-read after EVERY later call
                                                              test_programme on the box kinds
    host-side copies Md, Mf, cfg and the weights block, rewritten by set_weights, set_t_blast and
      set_params                                              test_setters_in_mid_life
    a refused call changes nothing of the above               test_refusals_leave_no_trace
    device globals shared by every handle of the process (g_* of mpcb_as.h, mpcb_split.hip,
      mpcb_box.hip)                                           test_three_handles_at_once
    the facade's last-solve tensors (get_control() and the others)   Life.remembers, after every call

qp_stats and mpcb_solve_iterate_pw / _pm: reading pw_impl (mpcb_capi.hip) shows that it neither
writes the statistics rows nor updates qp_stats_rows, so such a solve does not count as "the last
solve" (include/mpcb.h says so); the box kinds run pw_solve, pw_null and pm_solve between a solve and
a later read of its statistics.

Not vacuous: test_fresh_solves_match_the_oracle holds the fresh B = 79 solves to the CPU oracle at
each kind's own acceptance of tests/test_gpu_config.py.  Nothing here faults by design: every access
lies inside an allocation the test owns, and every refused call is one mpcb_capi.hip refuses before
any launch.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_call as ab   # noqa: E402
import history_calls as hc   # noqa: E402
import test_gpu_abi as ga   # noqa: E402
import test_gpu_config as gc   # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -4


# ------------------------------------------------------------------------------ the table itself
def test_first_calls_of_the_lazy_workspaces():
    """From PROGRAMME and SCHEDULE alone: for every kind and each workspace it allocates lazily, the
    first row that reaches it runs at B = 1 in one order and at B = 79 in the other; every row has
    another predecessor in order 2; every batch of the schedule is used."""
    assert sorted(hc.SCHEDULE) == [1, 3, 6, 7, 64, 65, 70, 79] and max(hc.SCHEDULE) == hc.MAXB
    assert len(set(hc.PROGRAMME)) == len(hc.PROGRAMME)
    for rows in hc.WORKSPACES.values():
        assert set(rows) <= set(hc.PROGRAMME)
    seen = set()
    for kd in hc.KINDS:
        first = {}
        for order in (1, 2):
            rows = [(n, B) for n, B in hc.plan(order) if kd.offers(n)]
            for ws in kd.workspaces:
                first[ws, order] = next(B for n, B in rows if n in hc.WORKSPACES[ws])
            seen |= {B for _, B in rows}
        for ws in kd.workspaces:
            assert {first[ws, 1], first[ws, 2]} == {1, hc.MAXB}, (kd.id, ws, first)
        assert kd.workspaces or kd.path == 'all'
    assert seen == set(hc.SCHEDULE)
    p1, p2 = [n for n, _ in hc.plan(1)], [n for n, _ in hc.plan(2)]
    pred = lambda p: {n: (p[i - 1] if i else None) for i, n in enumerate(p)}   # noqa: E731
    assert all(pred(p1)[n] != pred(p2)[n] for n in hc.PROGRAMME)
    # solve with and without trajectories stay neighbours: the alternation the fp32 box's own U needs
    assert abs(p1.index('solve') - p1.index('solve_nt')) == 1


# ------------------------------------------------------------------------------ not vacuous
@pytest.mark.parametrize('kd', hc.KINDS, ids=hc.KIND_IDS)
def test_fresh_solves_match_the_oracle(kd):
    """The fresh B = 79 ``solve`` and ``solve_iterate`` of each kind against the CPU oracle at the
    kind's own acceptance (test_gpu_config._accept_free / _accept_box / _accept17); on the box kinds
    at least 10 % of the oracle's input entries lie on a bound, and on ``box_ipm`` at least one
    instance went through the interior point."""
    i = {k: None if v is None else v.cpu().numpy().astype(np.float64) for k, v in hc.data(kd).items()
         if k in ('x0', 'xref', 'uref', 'wind')}
    for name, mode in (('solve', 'rollout'), ('solve_iterate', 'iterate')):
        o, spec = ga._oracle(kd, mode)
        r = {k: (v.astype(np.float64) if v.dtype.kind == 'f' else v) for k, v in hc.fresh(kd, 'base', name, hc.MAXB).items()}
        tag = f'{kd.id} {name} B={hc.MAXB}'
        assert (o['status'] == 0).all()
        if kd.boxed:
            frac = gc._on_bound(o['U'], spec.lbu, spec.ubu).mean()
            print(f'{tag}: oracle has {100 * frac:.0f} % of U on a bound')
            assert frac >= 0.10
        if kd.model == 17:
            gc._accept17(tag, o, spec, i['x0'], i['xref'], i['uref'], r['u0'], r['X'], r['U'], r['status'], kd.path, kd.dtype)
        elif kd.boxed:
            if kd.path == 'box_ipm':
                assert int(o['fallback'].sum()) >= 1
            gc._accept_box(tag, o, spec, i, r['u0'], r['X'], r['U'], r['status'], kd.dtype)
            assert (r['qp_stats'][:, 0] >= 1).all()
        else:
            gc._accept_free(tag, o, r['u0'], r['X'], r['U'], r['status'], kd.dtype)


# ------------------------------------------------------------------------------ the programme
@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('kd', hc.KINDS, ids=hc.KIND_IDS)
def test_programme(kd, order):
    """The programme twice on one new handle, beginning with ``order`` and then the other order (so
    that each lazy workspace is born at B = 1 in one test and at B = 79 in the other): every output of
    every call equals the fresh handle's, and after every call qp_stats and the getters still
    belong to the last solve (history_calls.Life)."""
    life = hc.Life(kd)
    try:
        life.run_plan(hc.plan(order))
        life.run_plan(hc.plan(3 - order))
    finally:
        life.close()
    assert len(life.done) == 2 * sum(kd.offers(n) for n in hc.PROGRAMME)


# ------------------------------------------------------------------------------ setters
@pytest.mark.parametrize('kd', hc.KINDS, ids=hc.KIND_IDS)
def test_setters_in_mid_life(kd):
    """After order 1: set_weights (the dense B-weights of tests/test_gpu_vjp_weights.py, fp32-rounded
    on f32 kinds), set_t_blast(2.5), on 17/6 set_params(p2) and later set_params(None); then every
    entry point once at B = 7 equals the fresh handle created with the final definition and differs
    from its own result before the setters (the rows of history_calls.INDEPENDENT read nothing a
    setter changes and must keep their bits)."""
    B = 7
    life = hc.Life(kd)
    try:
        life.run_plan(hc.plan(1))
        rows = [n for n in hc.PROGRAMME if kd.offers(n)]
        m = life.m
        before = {n: hc.run(m, kd, n, B) for n in rows}
        life.last_solve = life.last_facade = None
        m.set_weights(**hc.weights_b(kd))
        m.set_t_blast(hc.T_BLAST)
        stages = ['final']
        if kd.model == 17:
            m.set_params(hc.data(kd)['p2'])
            stages = ['final_p2', 'final']
        prev = before
        for defn in stages:
            if defn == 'final' and kd.model == 17:
                m.set_params(None)
            life.defn = defn
            now = {n: life.do(n, B) for n in rows}
            for n in rows:
                if n in hc.INDEPENDENT:
                    hc.same(now[n], before[n], f'{kd.id} {n}: reads nothing a setter changes')
                else:
                    assert hc.differs(now[n], before[n]), f'{kd.id} {n} {defn}: the setters did not reach it'
                    assert prev is before or hc.differs(now[n], prev[n]), f'{kd.id} {n}: set_params(None) did not reach it'
            prev = now
    finally:
        life.close()


# ------------------------------------------------------------------------------ refusals
REFUSAL_KINDS = [hc.kind(12, 'fused', 'f64'), hc.kind(12, 'box', 'f32'), hc.kind(17, 'input', 'f64')]


def _sentinel_outs(kd, m, B):
    N = kd.N
    return dict(u0=ab.guarded((B, m.nu), m.dtype), X=ab.guarded((B, N + 1, m.nx), m.dtype, 16),
                U=ab.guarded((B, N, m.nu), m.dtype, 16), status=ab.guarded((B,), torch.int32))


@pytest.mark.parametrize('kd', REFUSAL_KINDS, ids=[k.id for k in REFUSAL_KINDS])
def test_refusals_leave_no_trace(kd):
    """Half of order 1, then calls that mpcb_capi.hip refuses before any launch (check_solve's batch
    and stride rules; mpcb_solve_iterate_pm's fp32-box rule; mpcb_qp_stats without a box;
    validate_config's symmetry rule in mpcb_set_weights; check_params after a short set_params), then
    the rest.  Each returns its documented code, leaves its sentinel-filled outputs untouched, and the
    calls that follow equal their fresh references; the getters and qp_stats still answer for the
    last accepted solve."""
    from mpc_blaster_amd._lib import MpcbError
    life = hc.Life(kd)
    try:
        rows = hc.plan(1)
        half = len(rows) // 2
        life.run_plan(rows[:half])
        m, D, raw = life.m, hc.data(kd), ab.Raw(life.m)
        version = (m._weights_version, m._model_version)
        big = m.max_batch + 1
        z = lambda *s: torch.zeros(s, dtype=m.dtype, device='cuda')   # noqa: E731
        N, nx, nu = kd.N, m.nx, m.nu
        # B = max_batch + 1, every buffer large enough for it
        outs = _sentinel_outs(kd, m, big)
        rc = raw.solve(big, z(big, nx), nx, z(1, N + 1, nx), 0, z(1, N, nu), 0, None, 0, outs['u0'], outs['X'], outs['U'],
                       outs['status'], iterate=True, xbar=z(big, N + 1, nx), ubar=z(big, N, nu))
        assert rc == E_INVALID and 'max_batch' in raw.error()
        # a negative stride
        B = 7
        outs7 = _sentinel_outs(kd, m, B)
        for over in (dict(x0_sb=-nx), dict(xref_sb=-1), dict(uref_sb=-1)):
            sb = dict(dict(x0_sb=nx, xref_sb=(N + 1) * nx, uref_sb=N * nu), **over)
            rc = raw.solve(B, D['x0'], sb['x0_sb'], D['xref'], sb['xref_sb'], D['uref'], sb['uref_sb'], None, 0, outs7['u0'],
                           outs7['X'], outs7['U'], outs7['status'])
            assert rc == E_INVALID and 'stride' in raw.error(), over
        if kd.model == 12 and kd.boxed and kd.dtype == 'f32':
            with pytest.raises(MpcbError, match='fp64'):
                m.solve_iterate(D['x0'][:B], D['xbar'][:B], D['ubar'][:B], D['xref'][:B], D['uref'][:B], model=D['model'][:B],
                                out=tuple(outs7[k].view for k in ('u0', 'X', 'U', 'status')))
        if not kd.boxed:
            st = ab.guarded((B, 2), torch.int32)
            assert raw.qp_stats(B, st) == E_UNSUPPORTED
            with pytest.raises(MpcbError):
                m.qp_stats(B)
            torch.cuda.synchronize()
            assert st.untouched()
        asym = np.array(hc.weights_b(kd)['Q'])
        asym[2, 5] += 1e-3
        with pytest.raises(MpcbError, match='symmetric'):
            m.set_weights(Q=asym)
        short = None
        if kd.model == 17:
            m.set_params(D['p'][:5])     # accepted: five rows for a call of seven
            short = (m._model_version,)
            with pytest.raises(MpcbError, match='parameter rows'):
                m.solve_iterate(D['x0'][:B], D['xbar'][:B], D['ubar'][:B], D['xref'][:B], D['uref'][:B],
                                out=tuple(outs7[k].view for k in ('u0', 'X', 'U', 'status')))
            m.set_params(D['p'])
        torch.cuda.synchronize()
        for group in (outs, outs7):
            for n, o in group.items():
                assert o.untouched(), f'a refused call wrote into {n}'
        assert m._weights_version == version[0]
        assert m._model_version == (version[1] if short is None else short[0] + 1)
        life.remembers(f'{kd.id} after the refusals')
        life.run_plan(rows[half:])
    finally:
        life.close()


# ------------------------------------------------------------------------------ several handles
def test_three_handles_at_once():
    """A 12/4 box f64 handle, a 12/4 row32 f32 handle and a 17/6 input f64 handle alive together,
    their calls alternating one each in turn through order 1: each call equals its fresh reference
    (which ran with no other handle's call in between).  Half-way the row32 handle is destroyed; the
    others carry on unchanged."""
    kinds = [hc.kind(12, 'box', 'f64'), hc.kind(12, 'row32', 'f32'), hc.kind(17, 'input', 'f64')]
    for kd in kinds:
        hc.data(kd)   # (its fresh handle lives and dies before the three are created)
    lives = [hc.Life(kd) for kd in kinds]
    try:
        rows = hc.plan(1)
        for k, (name, B) in enumerate(rows):
            if k == len(rows) // 2:
                lives[1].close()
                del lives[1]
            for life in lives:
                if life.kd.offers(name):
                    life.do(name, B)
        assert len(lives) == 2 and all(len(life.done) >= 7 for life in lives)
    finally:
        for life in lives:
            life.close()
