"""tests/simvjp17_ref.py (the NumPy references of mpcb_sim_step_vjp17 and of the 17/6 closed loop)
against central differences of the oracle, the closed form of the 24 Jacobian entries, the frozen
cases that tests/test_gpu_simvjp17.py uses, and the declarations of the entry points.  No GPU.

Differences: Richardson-extrapolated central quotients (4 D(h/2) - D(h)) / 3 of g . rk4_step17 over
one entry of x, u or p at a time, absolute steps 1e-2 and 5e-3, on the first 8 instances of the
frozen draw.  The quotients measure themselves: the step pairs (1e-2, 5e-3) and (5e-3, 2.5e-3) are
compared per block in the metric of tests/simvjp17_ref.py ``blockerr``, asserted <= 1e-9, and the
reference is held to max(1e-12, 10 x that measured figure).

Measured (printed by the tests): self-agreement gx 1.6e-11, gu 1.3e-11, gJ 7.5e-12, gtb 4.6e-10;
reference against differences gx 1.7e-11, gu 3.8e-12, gJ 3.8e-12, gtb 1.2e-10; closed form against
the reference 7.3e-17 absolute.  Frozen loop case: status 0, identical active sets at every +- point,
149 of 162 components clamped with the box (50 of the 54 applied ones), quotient self-agreement
5.3e-11 (boxed) and 2.9e-11 (unboxed), gap between the quotients and the reference's own adjoint
2.0e-10 (boxed) and 6.3e-11 (unboxed), K = 4.5.
"""
import functools
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simvjp17_ref as s17   # noqa: E402

from oracle.full import default_p25, rk4_step17   # noqa: E402
from oracle.model import Params   # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 8
T = 2.0 / 60.0
P = Params()
SELF_BOUND = 1e-9


@functools.lru_cache(maxsize=None)
def draw():
    d = {k: v[:B].copy() for k, v in s17.step_case().items()}
    for a in d.values():
        a.setflags(write=False)
    d['ref'] = s17.simvjp17_ref(d['x'], d['u'], d['g'], T, P, d['p'])
    return d


def _richardson(d, which, h):
    """[B, n] quotients of g . rk4_step17 over the entries of ``which`` in ('x', 'u', 'p') at steps h, h/2."""
    n = d[which].shape[1]
    out = np.empty((B, n))
    for i in range(n):
        q = []
        for s in (h, 0.5 * h):
            v = []
            for sgn in (1.0, -1.0):
                a = {k: d[k].copy() for k in ('x', 'u', 'p')}
                a[which][:, i] += sgn * s
                v.append((d['g'] * rk4_step17(a['x'], a['u'], a['p'], T, P)).sum(axis=1))
            q.append((v[0] - v[1]) / (2.0 * s))
        out[:, i] = (4.0 * q[1] - q[0]) / 3.0
    return out


@functools.lru_cache(maxsize=None)
def _quotients(h):
    d = draw()
    return s17.blocks(dict(gx=_richardson(d, 'x', h), gu=_richardson(d, 'u', h), gparams=_richardson(d, 'p', h)))


def test_reference_matches_central_differences():
    ref = s17.blocks(draw()['ref'])
    q1, q2 = _quotients(1e-2), _quotients(5e-3)
    for k in s17.BLOCKS:
        own = s17.blockerr(q2[k], q1[k]).max()
        err = s17.blockerr(ref[k], q1[k]).max()
        bound = max(1e-12, 10.0 * own)
        print(f'{k}: quotient self-agreement {own:.2e}/{SELF_BOUND:.0e}, reference against differences {err:.2e}/{bound:.1e}')
        assert own <= SELF_BOUND and err <= bound, (k, own, err)


def test_closed_form_of_the_jacobian_entries():
    """Nothing reads the POC states: gJp, gJe, gJa follow from the step's increment (the form the
    device uses) and equal the forward-mode reference to rounding, for per-instance and for
    broadcast parameters."""
    d = draw()
    for p, ref in ((d['p'], d['ref']), (d['p'][:1], s17.simvjp17_ref(d['x'], d['u'], d['g'], T, P, d['p'][:1]))):
        e = np.abs(s17.closed_form(d['x'], d['u'], d['g'], T, P, p) - ref['gparams'][:, :24]).max()
        print(f'closed form against the forward-mode reference: {e:.2e} (|ref| {np.abs(ref["gparams"][:, :24]).max():.3g})')
        assert e <= 1e-15


def test_every_block_of_the_frozen_draw_is_above_the_floor():
    """The metric has no floor of 1, so no block of the draw may be tiny: per-instance, broadcast and
    default parameters, all BMAX instances."""
    c = s17.step_case()
    for tag, p in (('per-instance', c['p']), ('broadcast', c['p'][:1]), ('defaults', default_p25())):
        ref = s17.blocks(s17.simvjp17_ref(c['x'], c['u'], c['g'], T, P, p))
        low = {k: float(np.abs(v).reshape(s17.BMAX, -1).max(axis=1).min()) for k, v in ref.items()}
        print(f'{tag}: smallest |ref|_inf per block ' + '  '.join(f'{k} {low[k]:.2e}' for k in s17.BLOCKS))
        assert min(low.values()) >= s17.REF_FLOOR


def test_entry_points_are_declared_and_bound():
    from mpc_blaster_amd import _lib
    txt = open(os.path.join(REPO, 'include', 'mpcb.h')).read()
    for name in ('mpcb_sim_step_p17', 'mpcb_sim_step_vjp17'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', txt)
        assert name in _lib.EXPORTS_17 and name not in _lib.EXPORTS
    assert set(_lib.EXPORTS) == set(re.findall(r'\b(mpcb_[a-z_]+)\s*\(', txt))
    assert re.search(r'#define\s+MPCB_ABI_VERSION\s+5\b', txt) and _lib.ABI_VERSION == 5
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in _lib.EXPORTS_17)
    assert len(lib.mpcb_sim_step_p17.argtypes) == len(lib.mpcb_sim_step.argtypes)   # params for wind
    assert len(lib.mpcb_sim_step_vjp17.argtypes) == len(lib.mpcb_sim_step_p17.argtypes) + 3   # gxn, two more outputs
    doc = txt[txt.index('Reverse mode of the 17/6 plant step'):txt.index('int mpcb_sim_step_vjp17')]
    assert 'Out of scope' in doc and 'params_sb == 0' in doc and 'No atomics' in doc


def test_stale_library_without_the_symbols_is_refused(tmp_path):
    """A library of ABI version 5 from before the two entry points is told apart by the missing
    symbol (the stub pattern of tests/test_pm_ref_cpu.py)."""
    import subprocess

    import pytest

    from mpc_blaster_amd import _lib
    names = [n for n in _lib.EXPORTS + _lib.EXPORTS_17 if n not in ('mpcb_abi_version', 'mpcb_last_error')]
    for leave_out in ('mpcb_sim_step_p17', 'mpcb_sim_step_vjp17'):
        src = tmp_path / f'{leave_out}.c'
        src.write_text(f'int mpcb_abi_version(void) {{ return {_lib.ABI_VERSION}; }}\n'
                       'const char* mpcb_last_error(void) { return ""; }\n'
                       + ''.join(f'int {n}(void) {{ return 0; }}\n' for n in names if n != leave_out))
        so = tmp_path / f'lib{leave_out}.so'
        subprocess.run(['gcc', '-shared', '-fPIC', str(src), '-o', str(so)], check=True)
        with pytest.raises(_lib.LibraryMissing, match=f'has no {leave_out}: rebuild it'):
            _lib.load(str(so))


def test_frozen_loop_case_of_the_gpu_test():
    """The conditions tests/test_gpu_simvjp17.py test_closed_loop_diff17 relies on: status 0
    everywhere, identical active sets at all +- points, clamped and free components in the boxed
    variant, quotients that agree with themselves and with the reference's own adjoint, and the
    recorded figures."""
    for box in (False, True):
        case = s17.loop17_case(box)
        _, _, U, st, fixed = s17.loop17_eval(case, case['theta'])
        assert not st.any()
        q1, same1 = s17.loop17_quotients(case)
        q2, same2 = s17.loop17_quotients(case, s17.LOOP17_STEPS[1:])
        assert same1 and same2
        own = float((np.abs(q2 - q1) / np.maximum(np.abs(q1), 1.0)).max())
        print(f'box={box}: clamped {int(fixed.sum())} of {fixed.size} (u0: {int(fixed[:, :, 0].sum())} of '
              f'{fixed[:, :, 0].size}), quotients {q1}, self-agreement {own:.2e}/{s17.LOOP17_SELF_BOUND:.0e} '
              f'(recorded {s17.LOOP17_SELF[box]:.1e})')
        assert own <= s17.LOOP17_SELF_BOUND and own <= 1.5 * s17.LOOP17_SELF[box]
        # the quotient is a reference for the derivative on the active set only as far as the oracle's
        # interior point is one (tests/simvjp17_ref.py LOOP17_PSEED): held against the reference's own adjoint
        g = s17.loop17_grad_ref(case)
        ips = [sum(float((g[k] * d[k]).sum()) for k in s17.LOOP17_KEYS) for d in case['dirs']]
        gap = max(abs(ip - q) / max(abs(q), 1.0) for ip, q in zip(ips, q1))
        print(f'box={box}: reference adjoint {ips}, gap to the quotients {gap:.2e}/{s17.LOOP17_GAP_BOUND:.1e} '
              f'(recorded {s17.LOOP17_GAP[box]:.1e})')
        assert gap <= s17.LOOP17_GAP_BOUND and gap <= 1.5 * s17.LOOP17_GAP[box]
        if box:
            assert fixed.any() and not fixed.all() and fixed[:, :, 0].any() and not fixed[:, :, 0].all()
            K = s17.loop17_k(case, q1)
            print(f'K = {K:.3g} (recorded {s17.LOOP17_K})')
            assert K <= 1.5 * s17.LOOP17_K
        else:
            assert not fixed.any()
