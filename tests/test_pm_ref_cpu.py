"""tests/pm_ref.py (the NumPy references of mpcb_sim_step_pm, mpcb_solve_iterate_pm and
mpcb_solve_gains_pm) against the batched oracle, the box case that tests/test_gpu_pm.py uses, and
the declaration of the three entry points.  No GPU.

With every record equal to the spec's own ``Params`` the per-instance loop runs the oracle's code
on a batch of one with the same numbers.  The plant step is element-wise over the batch and is
asserted EXACTLY equal; the solve and the gains go through batched ``einsum`` / ``linalg.solve``
calls whose summation order may depend on the batch size, so they are asserted to 1e-12 (the bound
of tests/test_pw_ref_cpu.py for the same comparison).
"""
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gains_ref import gains_ref   # noqa: E402
from pm_ref import (MODEL_REC, pack_params, params_of, pm_gains_ref, pm_models, pm_sim_ref,   # noqa: E402
                    pm_solve_ref)
from pw_ref import no_early_handover, pw_weights   # noqa: E402
from vjp_ref import vjp_case   # noqa: E402

from oracle.ocp import OcpSpec, mpc_solve   # noqa: E402
from oracle.rk4 import rk4_step   # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the frozen box case of tests/test_gpu_pm.py: tests/vjp_ref.py vjp_case (seed 1004), the input box
# [5, 40] of the other box tests, vehicles pm_models(seed 21); the device's cap is 48 passes
BOX_B, BOX_N, BOX_SEED, AS_CAP = 8, 8, 21, 48
LB, UB = np.full(4, 5.0), np.full(4, 40.0)
ENTRY_POINTS = ('mpcb_sim_step_pm', 'mpcb_solve_iterate_pm', 'mpcb_solve_gains_pm')


@functools.lru_cache(maxsize=None)
def box_case():
    """(spec, case, models, reference solve) of the frozen box case; never modified."""
    spec = OcpSpec(N=BOX_N, lbu=LB, ubu=UB)
    c = vjp_case(BOX_B, BOX_N, spec)
    M = pm_models(BOX_B, spec, BOX_SEED)
    r = pm_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, M)
    for a in list(c.values()) + [M] + list(r.values()):
        if a is not None:
            a.setflags(write=False)
    return spec, c, M, r


def test_record_round_trip_and_vehicle_draw():
    spec = OcpSpec(N=3)
    rec = pack_params(spec.params)
    assert rec.shape == (MODEL_REC,)
    P = params_of(rec, spec.params)
    assert P.mass == spec.params.mass and P.g == spec.params.g and np.array_equal(P.J, spec.params.J)
    M = pm_models(6, spec)
    assert np.array_equal(M, pm_models(9, spec)[:6])   # instance b's draw does not depend on B
    J = M[:, 5:].reshape(-1, 3, 3)
    assert np.array_equal(J, np.swapaxes(J, 1, 2)) and np.linalg.eigvalsh(J).min() > 0
    assert np.abs(J[:, 0, 1]).min() > 0 and np.abs(J[:, 0, 2]).min() > 0 and np.abs(J[:, 1, 2]).min() > 0   # dense
    r = M[:, 0] / spec.params.mass
    assert r.min() >= 0.8 and r.max() <= 1.25 and M[:, 4].min() >= 0 and M[:, 4].max() <= 5.0
    for i, v in ((1, spec.params.lx), (2, spec.params.ly), (3, spec.params.c)):
        assert (M[:, i] / v).min() >= 0.9 and (M[:, i] / v).max() <= 1.1


@pytest.mark.parametrize('box', [False, True])
def test_equal_records_reproduce_the_batched_oracle(box):
    """Exactly for the plant step, to 1e-12 for the solve and the gains (module docstring)."""
    B, N = 6, 5
    spec = OcpSpec(N=N, lbu=LB if box else None, ubu=UB if box else None)
    c = vjp_case(B, N, spec, 'sine', True)
    M = np.tile(pack_params(spec.params)[None], (B, 1))
    # plant step
    u = c['ubar'][:, 0]
    assert np.array_equal(pm_sim_ref(c['x0'], u, spec.dt, spec, M, c['wind']),
                          rk4_step(c['x0'], u, spec.dt, spec.params, c['wind']))
    assert np.array_equal(pm_sim_ref(c['x0'], u, spec.dt, spec, M[:1]), rk4_step(c['x0'], u, spec.dt, spec.params))
    # solve
    with no_early_handover():
        o = mpc_solve(c['x0'], c['xref'], c['uref'], spec, wind=c['wind'], mode='iterate', xbar=c['xbar'],
                      ubar=c['ubar'])
    r = pm_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, M, wind=c['wind'])
    none = pm_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, None, wind=c['wind'])
    assert not o['fallback'].any() and not r['fallback'].any()
    for k in ('u0', 'X', 'U'):
        assert np.abs(r[k] - o[k]).max() <= 1e-12 * max(1.0, np.abs(o[k]).max()), k
        assert np.array_equal(r[k], none[k]), k
    assert np.array_equal(r['status'], o['status']) and np.array_equal(r['iters'], o['iters'])
    # gains
    fixed = np.random.default_rng(5).random((B, N, 4)) < 0.5
    for fx in (None, fixed):
        g, go = pm_gains_ref(c['xbar'], c['ubar'], fx, spec, M, c['wind']), gains_ref(c['xbar'], c['ubar'], fx, spec,
                                                                                        c['wind'])
        assert g['ok'].all()
        for k in ('K', 'P0'):
            assert np.abs(g[k] - go[k]).max() <= 1e-12 * max(1.0, np.abs(go[k]).max()), k


def test_vehicles_move_the_solution_on_every_instance():
    B, N = 6, 5
    spec = OcpSpec(N=N)
    c = vjp_case(B, N, spec, 'sine', True)
    M = pm_models(B, spec)
    o = mpc_solve(c['x0'], c['xref'], c['uref'], spec, wind=c['wind'], mode='iterate', xbar=c['xbar'], ubar=c['ubar'])
    p = pm_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, M, wind=c['wind'])
    d = np.abs(p['U'] - o['U']).reshape(B, -1).max(axis=1) / np.maximum(np.abs(o['U']).reshape(B, -1).max(axis=1), 1.0)
    print(f'per-instance vehicles against the shared one: relative move of U per instance {d.round(4).tolist()}')
    assert d.min() > 1e-3
    # ... and combine with per-instance weights
    Q, R, QN = pw_weights(B, spec)
    pq = pm_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, M, Q, R, QN, c['wind'])
    assert np.abs(pq['U'] - p['U']).reshape(B, -1).max(axis=1).min() > 1e-3
    # the plant step and the gains move too
    u = c['ubar'][:, 0]
    xs, x1 = pm_sim_ref(c['x0'], u, spec.dt, spec, M), rk4_step(c['x0'], u, spec.dt, spec.params)
    assert (np.abs(xs - x1).max(axis=1) / np.maximum(np.abs(x1).max(axis=1), 1.0)).min() > 1e-3
    g, g1 = pm_gains_ref(c['xbar'], c['ubar'], None, spec, M), gains_ref(c['xbar'], c['ubar'], None, spec)
    assert np.abs(g['K'] - g1['K']).reshape(B, -1).max(axis=1).min() > 1e-3


def test_frozen_box_case_of_the_gpu_test():
    """The reference alone: converged within the device's cap, no hand-over to the interior point,
    at least one clamped component on most instances."""
    spec, c, M, r = box_case()
    assert np.all(r['status'] == 0) and not r['fallback'].any() and r['iters'].max() <= AS_CAP
    fixed = (r['U'] <= LB + 1e-9) | (r['U'] >= UB - 1e-9)
    per = fixed.sum(axis=(1, 2))
    print(f'pm box case: reference passes {r["iters"].tolist()}, clamped components per instance {per.tolist()}')
    assert (per > 0).sum() > BOX_B // 2
    assert r['iters'].max() > 1   # the active set does iterate


def test_entry_points_are_declared_and_bound():
    from mpc_blaster_amd import _lib
    txt = open(os.path.join(REPO, 'include', 'mpcb.h')).read()
    declared = set(re.findall(r'\b(mpcb_[a-z_]+)\s*\(', txt))
    for name in ENTRY_POINTS:
        assert name in declared and name in _lib.EXPORTS and name in _lib.EXPORTS_PM
        assert re.search(r'\bint\s+' + name + r'\s*\(', txt)
    assert set(_lib.EXPORTS) == declared
    assert re.search(r'#define\s+MPCB_MODEL_REC\s+14\b', txt) and _lib.MODEL_REC == MODEL_REC == 14
    assert re.search(r'#define\s+MPCB_ABI_VERSION\s+5\b', txt) and _lib.ABI_VERSION == 5
    lib = _lib.load()
    assert len(lib.mpcb_sim_step_pm.argtypes) == len(lib.mpcb_sim_step.argtypes) + 2
    assert len(lib.mpcb_solve_iterate_pm.argtypes) == len(lib.mpcb_solve_iterate_pw.argtypes) + 2
    assert len(lib.mpcb_solve_gains_pm.argtypes) == len(lib.mpcb_solve_gains.argtypes) + 2
    # the header says what the library cannot check and what is out of scope
    doc = txt[:txt.index('#define MPCB_MODEL_REC')]
    doc = doc[doc.rindex('/*'):]
    assert 'symmetric positive definite' in doc and 'Out of scope' in doc and 'model_sb == 0' in doc


def test_stale_library_without_the_symbols_is_refused(tmp_path):
    """The three exports are optional at load the way mpcb_solve_gains is: a library of ABI version
    5 from before them is told apart by the missing symbol (the stub pattern of
    tests/test_gains_ref_cpu.py)."""
    import subprocess

    from mpc_blaster_amd import _lib
    names = [n for n in _lib.EXPORTS + _lib.EXPORTS_17 if n not in ('mpcb_abi_version', 'mpcb_last_error')]
    for leave_out in ENTRY_POINTS:
        src = tmp_path / f'{leave_out}.c'
        src.write_text(f'int mpcb_abi_version(void) {{ return {_lib.ABI_VERSION}; }}\n'
                       'const char* mpcb_last_error(void) { return ""; }\n'
                       + ''.join(f'int {n}(void) {{ return 0; }}\n' for n in names if n != leave_out))
        so = tmp_path / f'lib{leave_out}.so'
        subprocess.run(['gcc', '-shared', '-fPIC', str(src), '-o', str(so)], check=True)
        with pytest.raises(_lib.LibraryMissing, match=f'has no {leave_out}: rebuild it'):
            _lib.load(str(so))
