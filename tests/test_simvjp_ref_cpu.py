"""tests/simvjp_ref.py (the NumPy references of mpcb_sim_step_vjp and of closed_loop_diff's forward
pass) against central differences of the oracle, the frozen closed-loop case that
tests/test_gpu_simvjp.py uses, and the declaration of the entry point.  No GPU.

Differences: Richardson-extrapolated central quotients (4 D(h/2) - D(h)) / 3 of g . rk4_step over one
entry at a time, relative steps 1e-3 and 5e-4 of max(|entry|, floor); floors 1e-2 for record entries
(zero off-diagonals of J move), 1 for wind, x and u.  Draw (seed 31): x in U(-0.5, 0.5), u in
U(0, 65), wind in U(-2, 2), g ~ N(0, 1), vehicles pm_models(B = 8).  The quotients measure
themselves: the step pairs (1e-3, 5e-4) and (5e-4, 2.5e-4) are compared in the relerr metric of
tests/test_gpu_vjp.py, asserted <= 1e-9, and the reference is held to 10 x that measured figure
(the factor covers the coarser pair's fourth-order term).

Measured: self-agreement gmodel+gwind 6.1e-11, gx+gu 1.2e-12; reference against differences
3.6e-11 and 5.2e-13 (printed by the tests).
"""
import functools
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simvjp_ref as sr   # noqa: E402
from pm_ref import params_of, pm_models   # noqa: E402
from test_gpu_vjp import relerr   # noqa: E402

from oracle.ocp import OcpSpec   # noqa: E402
from oracle.rk4 import rk4_step   # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 8
SELF_BOUND = 1e-9


@functools.lru_cache(maxsize=None)
def draw():
    rng = np.random.default_rng(31)
    spec = OcpSpec(N=3)
    d = dict(x=rng.uniform(-0.5, 0.5, (B, 12)), u=rng.uniform(0.0, 65.0, (B, 4)), wind=rng.uniform(-2.0, 2.0, (B, 3)),
             g=rng.standard_normal((B, 12)), M=pm_models(B, spec))
    for a in d.values():
        a.setflags(write=False)
    d['spec'] = spec
    d['ref'] = sr.simvjp_ref(d['x'], d['u'], d['g'], spec.dt, spec, d['M'], d['wind'])
    return d


def _phi(d, b, x, u, rec, w):
    return float(d['g'][b] @ rk4_step(x[None], u[None], d['spec'].dt, params_of(rec, d['spec'].params), w[None])[0])


def _richardson(d, which, floor, h):
    """[B, n] quotients over the entries of ``which`` in ('x', 'u', 'M', 'wind') at steps h, h/2."""
    n = d[which].shape[1]
    out = np.empty((B, n))
    for b in range(B):
        base = dict(x=d['x'][b], u=d['u'][b], M=d['M'][b], wind=d['wind'][b])
        for i in range(n):
            q = []
            for hh in (h, 0.5 * h):
                e = hh * max(abs(base[which][i]), floor)
                v = []
                for sgn in (1.0, -1.0):
                    a = dict(base)
                    a[which] = base[which].copy()
                    a[which][i] += sgn * e
                    v.append(_phi(d, b, a['x'], a['u'], a['M'], a['wind']))
                q.append((v[0] - v[1]) / (2.0 * e))
            out[b, i] = (4.0 * q[1] - q[0]) / 3.0
    return out


def _against_differences(pairs, tag):
    d = draw()
    fd = np.concatenate([_richardson(d, w, fl, 1e-3) for w, _, fl in pairs], axis=1)
    fd2 = np.concatenate([_richardson(d, w, fl, 5e-4) for w, _, fl in pairs], axis=1)
    ref = np.concatenate([d['ref'][k] for _, k, _ in pairs], axis=1)
    self_agree = relerr(fd, fd2).max()
    err = relerr(ref, fd).max()
    print(f'{tag}: self-agreement of the differences {self_agree:.2e} (<= {SELF_BOUND:.0e}), reference against '
          f'differences {err:.2e} (<= {10 * self_agree:.2e})')
    assert self_agree <= SELF_BOUND
    assert err <= 10.0 * self_agree


def test_gmodel_gwind_against_differences():
    _against_differences((('M', 'gmodel', 1e-2), ('wind', 'gwind', 1.0)), 'gmodel, gwind')


def test_gx_gu_against_differences():
    """Guards the transposition and the indexing of A^T g, B^T g."""
    _against_differences((('x', 'gx', 1.0), ('u', 'gu', 1.0)), 'gx, gu')


def test_frozen_loop_case_of_the_gpu_test():
    """loop_ref at B = 3, N = 3, nsim = 3, warm_start=False on the frozen boxed case (seed
    simvjp_ref.LOOP_SEED, box [5, 40]): some u0 component is clamped in some step, every status is 0,
    the active sets of all solves are those of the centre at every +- point of the quotients the GPU
    test uses, and those quotients agree with the pair of half the steps within LOOP_SELF_BOUND.
    Measured self-agreement: boxed 3.7e-11, unboxed twin 9.2e-11 (printed; recorded as LOOP_SELF)."""
    for box in (True, False):
        c = sr.loop_case(box)
        _, X, U, st, fixed = sr.loop_eval(c, c['theta'])
        assert not st.any()
        if box:
            lb, ub = sr.LOOP_LB, sr.LOOP_UB
            assert np.array_equal(fixed[:, :, 0], (U <= lb) | (U >= ub))
            assert fixed[:, :, 0].any() and not fixed[:, :, 0].all()
        q1, same1 = sr.loop_quotients(c)
        q2, same2 = sr.loop_quotients(c, sr.LOOP_STEPS[1:])
        agree = (np.abs(q1 - q2) / np.maximum(np.abs(q1), 1.0)).max()
        print(f'loop case box={box}: clamped u0 components per instance and step '
              f'{fixed[:, :, 0].sum(axis=2).tolist()}, quotients {q1.round(4).tolist()}, self-agreement {agree:.2e}')
        assert same1 and same2
        assert agree <= sr.LOOP_SELF_BOUND and sr.LOOP_SELF[box] <= sr.LOOP_SELF_BOUND


def test_loop_ref_warm_start_moves_the_iterate():
    c = sr.loop_case(True)
    th = c['theta']
    de = lambda D: np.stack([np.diag(v) for v in D])   # noqa: E731
    a = [sr.loop_ref(th['x0'], th['xref'], th['uref'], sr.LOOP_NSIM, c['xbar'], c['ubar'], c['spec'], de(th['Q']),
                     de(th['R']), de(th['QN']), th['plant_model'], warm_start=ws) for ws in (True, False)]
    assert np.array_equal(a[0][0][:, :2], a[1][0][:, :2])      # the first step is the same solve
    assert not np.array_equal(a[0][0][:, 2:], a[1][0][:, 2:])


def test_entry_point_is_declared_and_bound():
    from mpc_blaster_amd import _lib
    txt = open(os.path.join(REPO, 'include', 'mpcb.h')).read()
    declared = set(re.findall(r'\b(mpcb_[a-z_]+)\s*\(', txt))
    assert 'mpcb_sim_step_vjp' in declared and 'mpcb_sim_step_vjp' in _lib.EXPORTS
    assert re.search(r'\bint\s+mpcb_sim_step_vjp\s*\(', txt)
    assert set(_lib.EXPORTS) == declared
    assert re.search(r'#define\s+MPCB_ABI_VERSION\s+5\b', txt) and _lib.ABI_VERSION == 5
    lib = _lib.load()
    # mpcb_sim_step_pm's arguments without x_out, then gxn and the four outputs
    assert len(lib.mpcb_sim_step_vjp.argtypes) == len(lib.mpcb_sim_step_pm.argtypes) + 4
    doc = txt[:txt.index('#define MPCB_MODEL_REC')]
    doc = doc[doc.rindex('/*'):]
    assert 'mpcb_sim_step_vjp' in doc
