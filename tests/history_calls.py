"""The call programme of tests/test_gpu_history.py: handle kinds, the fixed programme table, one
function per entry point, and the reference of record (the same call on a fresh handle); a helper,
not a test.

A *kind* is a handle configuration: a path of tests/test_gpu_config.py's PATHS table or a 17/6
bounds setting, a dtype, and optionally MPCB_CHUNK=64, under the default problem definition
(tests/test_gpu_abi.py's _cfg_fields).  Every handle has max_batch = MAXB (the ``thread`` path keeps
its 16385).  A *definition* is what the setters can change: ``base`` (the config as created; 17/6:
``set_params(p)`` of the draw), ``final`` (the B-weights of tests/test_gpu_vjp_weights.py and
T_blast = 2.5 in the config; 17/6: default parameters) and ``final_p2`` (17/6: ``final`` plus
``set_params(p2)``).

Every call takes the first B rows of one 79-instance draw per (model, dtype) (``data``), so a call is
the triple (entry point, definition, B) and nothing else.  X and U, which the products, the gains and
``evaluate`` read as inputs, are those of a fresh handle's B = 79 ``solve_iterate`` under ``base``.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alt_config as ac   # noqa: E402
import test_gpu_abi as ga   # noqa: E402
import test_gpu_config as gc   # noqa: E402

import torch   # noqa: E402

MAXB = 79
# B: 79 the whole handle, 1 a single instance, 70 a chunk plus six on the chunked kinds, 6 a ragged
# quad of 2, 64 exactly one chunk, 7 a ragged quad of 3, 65 a second chunk of one instance, 3 a
# ragged quad of 3
SCHEDULE = (79, 1, 70, 6, 64, 7, 65, 3)

# Row k takes SCHEDULE[k % 8] in order 1; order 2 is the table reversed with the schedule rotated by
# three (``plan``).  A row a kind does not offer is skipped and keeps its slot, so the batches below
# hold for every kind.  The order is chosen so that each lazily allocated workspace (WORKSPACES) sees
# its first call at B = 1 in one order and at B = 79 in the other; test_gpu_history.py asserts that
# from this table.
PROGRAMME = ('pm_gains', 'vjp', 'pw_vjp', 'gains_fixed', 'gains_U', 'vjp_w', 'sim_step', 'solve_iterate', 'evaluate',
             'pm_solve', 'sim_step_pm', 'pw_solve', 'gen_inputs', 'pw_null', 'solve', 'solve_nt', 'sim_step_vjp',
             'linearize', 'histogram')
# struct mpcb_handle's workspaces that the first call of an entry point allocates -> the rows that
# reach it (mpcb_capi.hip: vjp_impl, gains_impl, pw_impl, ensure_vjp17_ws)
WORKSPACES = {'vjp_scratch': ('vjp', 'vjp_w', 'pw_vjp'), 'gains_scratch': ('gains_U', 'gains_fixed', 'pm_gains'),
              'pw_scratch': ('pw_solve', 'pw_null', 'pm_solve'),
              'vjp17_scratch': ('vjp', 'vjp_w', 'gains_U', 'gains_fixed')}
SOLVES = ('solve', 'solve_nt', 'solve_iterate')                 # the last solve of mpcb_qp_stats
FACADE_SOLVES = SOLVES + ('pw_solve', 'pw_null', 'pm_solve')    # the last solve of get_control() and the others
ONLY12 = ('pm_gains', 'pw_vjp', 'pm_solve', 'sim_step_pm', 'pw_solve', 'gen_inputs', 'pw_null', 'sim_step_vjp', 'histogram')
# rows that read nothing a setter changes: the record carries the whole vehicle; no model at all
INDEPENDENT = ('sim_step_pm', 'gen_inputs', 'histogram')
TOL17 = 1e-4    # the 17/6 active-set tolerance of the products and gains (required on f32)


class Kind:
    def __init__(self, model, path, dtype, chunk=False):
        self.model, self.path, self.dtype, self.chunk = model, path, dtype, chunk
        self.N, self.B = (6 if model == 12 else 7), MAXB      # (B: the oracle's batch, test_gpu_abi._oracle)
        self.boxed = path in ga.BOXED12 if model == 12 else path != 'none'
        self.id = f'{model}-{path}-{dtype}' + ('-chunk64' if chunk else '')

    def offers(self, name):
        if self.model == 17:
            if name in ONLY12:
                return False
            return not (self.path == 'all' and name in WORKSPACES['vjp17_scratch'])   # the state box: refused
        # mpcb_solve_iterate_pw / _pm with the input box need an fp64 handle
        return not (self.boxed and self.dtype == 'f32' and name in WORKSPACES['pw_scratch'])

    @property
    def workspaces(self):
        if self.model == 17:
            return () if self.path == 'all' else ('vjp17_scratch',)
        return tuple(w for w in ('vjp_scratch', 'gains_scratch', 'pw_scratch')
                     if any(self.offers(n) for n in WORKSPACES[w]))


KINDS = [Kind(12, 'fused', 'f64'), Kind(12, 'row32', 'f32'), Kind(12, 'small', 'f64'), Kind(12, 'single', 'f64'),
         Kind(12, 'thread', 'f32'), Kind(12, 'box', 'f64'), Kind(12, 'box', 'f32'), Kind(12, 'box_ipm', 'f64'),
         Kind(12, 'fused', 'f64', chunk=True),
         Kind(17, 'none', 'f64'), Kind(17, 'input', 'f64'), Kind(17, 'input', 'f32'), Kind(17, 'all', 'f64'),
         Kind(17, 'input', 'f64', chunk=True)]
KIND_IDS = [k.id for k in KINDS]


def kind(model, path, dtype, chunk=False):
    return next(k for k in KINDS if (k.model, k.path, k.dtype, k.chunk) == (model, path, dtype, chunk))


def plan(order):
    """[(row name, B)] of order 1 (as listed) or 2 (reversed, the schedule rotated by three)."""
    rows = PROGRAMME if order == 1 else PROGRAMME[::-1]
    shift = 0 if order == 1 else 3
    return [(name, SCHEDULE[(k + shift) % len(SCHEDULE)]) for k, name in enumerate(rows)]


# ------------------------------------------------------------------------------ definitions
def weights_b(kd):
    from test_gpu_vjp_weights import _weights_b
    wb = _weights_b() if kd.model == 12 else _weights_b(17, 6, seed=29)
    return {k: ac._r32(v) if kd.dtype == 'f32' else v for k, v in wb.items()}


T_BLAST = 2.5


def make(kd, defn='base'):
    """A new handle of the kind under a definition: the environment switches are set for the
    construction alone (they are read there and never by a call)."""
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    cfg = ga._cfg_fields(kd)
    if defn != 'base':
        cfg = dict(cfg, t_blast=T_BLAST, **weights_b(kd))
    with pytest.MonkeyPatch.context() as mp:
        if kd.chunk:
            mp.setenv('MPCB_CHUNK', '64')
        if kd.model == 12:
            return gc._handle(kd.path, kd.N, MAXB, kd.dtype, mp, **cfg)
        m = BatchedMPC(MPCConfig.full(N=kd.N, dtype=kd.dtype, **cfg), max_batch=MAXB)
    if defn == 'base':
        m.set_params(_d(kd)['p'])
    elif defn == 'final_p2':
        m.set_params(_d(kd)['p2'])
    return m


# ------------------------------------------------------------------------------ inputs
def _tdt(kd):
    return torch.float64 if kd.dtype == 'f64' else torch.float32


def _dev(kd, a):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda').to(_tdt(kd)).contiguous()


@functools.lru_cache(maxsize=None)
def _data(model, dtype):
    """The one 79-instance draw of a (model, dtype), on the device; never modified."""
    from mpc_blaster_amd import MPCConfig
    kd = Kind(model, 'fused' if model == 12 else 'none', dtype)
    inp = dict(gc._inputs(kd.N, MAXB, dtype)) if model == 12 else dict(ga._inputs17(kd.N, MAXB, dtype))
    nx, nu, N = (12, 4, kd.N) if model == 12 else (17, 6, kd.N)
    rng = np.random.default_rng(41)
    inp['gX'], inp['gU'] = rng.standard_normal((MAXB, N + 1, nx)), rng.standard_normal((MAXB, N, nu))
    inp['gxn'] = rng.standard_normal((MAXB, nx))
    D = {k: _dev(kd, v) for k, v in inp.items()}
    D['u'] = D['ubar'][:, 0].contiguous()
    D['fixed'] = torch.as_tensor((rng.random((MAXB, N, nu)) < 0.2).astype(np.uint8), device='cuda')
    if model == 12:
        c = MPCConfig()
        D['Qd'] = _dev(kd, np.diag(c.Q) * rng.uniform(0.7, 1.3, (MAXB, 12)))
        D['Rd'] = _dev(kd, np.diag(c.R) * rng.uniform(0.7, 1.3, (MAXB, 4)))
        D['QNd'] = _dev(kd, np.diag(c.QN) * rng.uniform(0.7, 1.3, (MAXB, 12)))
        rec = np.r_[c.mass, c.lx, c.ly, c.c, 3.0, np.asarray(c.J, dtype=np.float64).reshape(9)]
        D['model'] = _dev(kd, rec * rng.uniform(0.8, 1.2, (MAXB, 14)))   # (a diagonal J stays diagonal)
    else:
        p2 = 1.1 * inp['p']
        p2[..., 24] = 3.0
        D['p2'] = _dev(kd, p2)
        D['wind'] = None
    return D


@functools.lru_cache(maxsize=None)
def data(kd):
    """``_data`` plus X and U of a fresh handle's B = 79 ``solve_iterate`` under ``base``."""
    D = dict(_data(kd.model, kd.dtype))
    D['X'] = D['U'] = None
    _DATA_BOOT[kd] = D
    try:
        r = fresh(kd, 'base', 'solve_iterate', MAXB)
    finally:
        del _DATA_BOOT[kd]
    D['X'], D['U'] = _dev(kd, r['X']), _dev(kd, r['U'])
    return D


_DATA_BOOT = {}   # (the draw without X and U, while ``data`` computes them)


def _d(kd):
    return _DATA_BOOT[kd] if kd in _DATA_BOOT else data(kd)


# ------------------------------------------------------------------------------ the calls
def _solve_out(m):
    return dict(u0=m._u0, X=m._X, U=m._U, status=m._status)


def call(m, kd, name, B):
    """Row ``name`` at batch B on handle ``m`` through ``BatchedMPC``: {output name: device tensor}."""
    D = _d(kd)
    s = lambda k: None if D.get(k) is None else D[k][:B]   # noqa: E731
    full = kd.model == 17
    w = {} if full else dict(wind=s('wind'))
    tol = dict(active_tol=TOL17) if full else {}
    ref = dict(X=s('X'), x_ref=s('xref'), u_ref=s('uref'), weights=True)
    pw = dict(Q=s('Qd'), R=s('Rd'), QN=s('QNd'))
    it = (s('x0'), s('xbar'), s('ubar'), s('xref'), s('uref'))
    if name == 'solve':
        m.solve(s('x0'), s('xref'), s('uref'), **w)
        return _solve_out(m)
    if name == 'solve_nt':
        m.solve(s('x0'), s('xref'), s('uref'), want_traj=False, **w)
        return _solve_out(m)
    if name == 'solve_iterate':
        m.solve_iterate(*it, **w)
        return _solve_out(m)
    if name == 'pw_solve':     # per-instance Q, R, QN
        m.solve_iterate(*it, **w, **pw)
        return _solve_out(m)
    if name == 'pw_null':      # R alone: Q and QN NULL fall back to the handle's
        m.solve_iterate(*it, **w, R=s('Rd'))
        return _solve_out(m)
    if name == 'pm_solve':     # a vehicle per instance, the handle's weights
        m.solve_iterate(*it, **w, model=s('model'))
        return _solve_out(m)
    if name == 'linearize':
        return dict(zip(('A', 'B', 'xn'), m.linearize(s('xbar'), s('ubar'), **w)))
    if name == 'evaluate':
        return m.evaluate(s('X'), s('U'), s('xref'), s('uref'), x0=s('x0'), stat=kd.path != 'all', **w)
    if name == 'vjp':
        return m.solve_iterate_vjp(s('xbar'), s('ubar'), gX=s('gX'), gU=s('gU'), U=s('U'), **w, **tol)
    if name == 'vjp_w':
        return m.solve_iterate_vjp(s('xbar'), s('ubar'), gX=s('gX'), gU=s('gU'), U=s('U'), **w, **tol, **ref)
    if name == 'pw_vjp':       # the per-instance-weight product, weight gradients included
        return m.solve_iterate_vjp(s('xbar'), s('ubar'), gX=s('gX'), gU=s('gU'), U=s('U'), **w, **ref, **pw)
    if name == 'gains_U':
        return m.solve_iterate_gains(s('xbar'), s('ubar'), U=s('U'), **w, **tol)
    if name == 'gains_fixed':
        return m.solve_iterate_gains(s('xbar'), s('ubar'), fixed=s('fixed'), **w)
    if name == 'pm_gains':
        return m.solve_iterate_gains(s('xbar'), s('ubar'), U=s('U'), **w, model=s('model'))
    if name == 'sim_step':
        return dict(xo=m.sim_step(s('x0'), s('u'), **w))
    if name == 'sim_step_pm':
        return dict(xo=m.sim_step(s('x0'), s('u'), **w, model=s('model')))
    if name == 'sim_step_vjp':   # without a record: the handle's vehicle, gmodel at its config
        return m.sim_step_vjp(s('x0'), s('u'), s('gxn'), **w, want=('gx', 'gu', 'gwind', 'gmodel'))
    if name == 'histogram':
        return dict(counts=m.histogram(D['U'][:B, 0].contiguous(), lo=0.0, hi=65.0, nbins=64))
    if name == 'gen_inputs':
        return m.gen_inputs(B, 11, id_offset=5, ref='sine', wind=True)
    raise KeyError(name)


def host(out):
    """{name: host array} of a call's outputs (None entries left out), once the device is idle."""
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in out.items() if v is not None}


def run(m, kd, name, B):
    """``call`` on the host, plus ``qp_stats`` read straight after a solve on the kinds that keep it."""
    r = host(call(m, kd, name, B))
    if name in SOLVES and kd.boxed:
        r['qp_stats'] = host(dict(s=m.qp_stats(B)))['s']
    return r


@functools.lru_cache(maxsize=None)
def fresh(kd, defn, name, B):
    """The reference of record: the same call on a handle of the same kind and definition that has
    made no other call.  One handle per distinct (kind, definition, call, B), then destroyed."""
    m = make(kd, defn)
    try:
        return run(m, kd, name, B)
    finally:
        m.close()


def same(got, want, tag):
    """Bit equality of every output (NaN payloads included), the first difference in the message."""
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    for n in want:
        a, b = got[n], want[n]
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, n, a.shape, b.shape, a.dtype, b.dtype)
        if a.tobytes() != b.tobytes():
            ne = ~((a == b) | (np.isnan(a) & np.isnan(b))) if a.dtype.kind == 'f' else a != b
            idx = np.argwhere(ne)
            raise AssertionError(f'{tag}: {n} differs from the fresh handle in {len(idx)} of {a.size} entries, first at '
                                 f'{idx[:4].tolist()}: {a[ne][:4]} against {b[ne][:4]}')


def differs(a, b):
    return any(a[n].tobytes() != b[n].tobytes() for n in a)


# ------------------------------------------------------------------------------ a handle's life
class Life:
    """A handle under test and what it must still remember: after every call the outputs equal the
    fresh handle's, ``qp_stats`` is still the last shared-weight solve's (mpcb_solve /
    mpcb_solve_iterate; a boxed mpcb_solve_iterate_pw / _pm in between does not count, include/mpcb.h)
    and ``get_control()`` and the others still return the last solve's tensors."""

    def __init__(self, kd, defn='base'):
        self.kd, self.defn, self.m = kd, defn, make(kd, defn)
        self.last_solve = self.last_facade = None   # (definition, name, B)
        self.done = []

    def do(self, name, B):
        kd = self.kd
        tag = f'{kd.id} call {len(self.done)} {name} B={B} after {self.done[-3:]}'
        r = run(self.m, kd, name, B)
        same(r, fresh(kd, self.defn, name, B), tag)
        if name in SOLVES:
            self.last_solve = (self.defn, name, B)
        if name in FACADE_SOLVES:
            self.last_facade = (self.defn, name, B)
        self.done.append(f'{name}@{B}')
        self.remembers(tag)
        return r

    def remembers(self, tag):
        kd, m = self.kd, self.m
        if kd.boxed and self.last_solve is not None:
            want = fresh(kd, *self.last_solve)['qp_stats']
            got = host(dict(s=m.qp_stats(self.last_solve[2])))['s']
            assert got.tobytes() == want.tobytes(), f'{tag}: qp_stats is no longer that of {self.last_solve}'
        if self.last_facade is not None:
            want = fresh(kd, *self.last_facade)
            got = host(dict(u0=m.get_control(), status=m.get_status(), X=m._X, U=m._U))
            if 'X' in got:
                assert m.get_state_trajectory() is m._X and m.get_input_trajectory() is m._U
            same(got, {k: v for k, v in want.items() if k != 'qp_stats'}, f'{tag}: the getters, last solve {self.last_facade}')

    def run_plan(self, rows):
        for name, B in rows:
            if self.kd.offers(name):
                self.do(name, B)

    def close(self):
        self.m.close()
