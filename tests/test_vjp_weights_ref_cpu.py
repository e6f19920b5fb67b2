"""tests/vjp_weights_ref.py (the NumPy reference of the weight gradients of mpcb_solve_vjp_w) against
central finite differences of the oracle's ``mpc_solve(mode='iterate')`` over every independent
entry of Q, R and QN, and the declaration of the two new entry points.  No GPU.

L = <gX, X> + <gU, U> with standard normal cotangents (tests/vjp_ref.py vjp_case).  For the entry
(i, j), i <= j, of a weight W the probe is W +- h D with the symmetric D = E_ij + E_ji and
h = 1e-4 sqrt(W_ii W_jj); the reference's prediction of (L+ - L-) / 2h is <g, D> = g_ij + g_ji.
L is not affine in the weights, so the central difference carries a truncation error of relative
order 1e-8 times the curvature: the bound is 1e-6 of the instance's largest predicted entry.  It is
asserted per output (gQ, gR and gQN each against its own largest entry), which is the stricter
reading; the figure against the largest entry of all three is printed beside it.  With the box
an instance counts by the rules of tests/test_vjp_ref_cpu.py: the oracle's active set is the same at
every probe and the active-set method solved it (no hand-over to the interior point).
"""
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alt_config as ac   # noqa: E402
from test_vjp_ref_cpu import _snap   # noqa: E402
from vjp_ref import vjp_case   # noqa: E402
from vjp_weights_ref import KEYS, vjp_weights_ref   # noqa: E402

from oracle.ocp import OcpSpec, mpc_solve   # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'gQ': 'Q', 'gR': 'R', 'gQN': 'QN'}
BOUND = 1e-6
REL_STEP = 1e-4


def _fd(c, spec, base):
    """Central differences of L over every independent weight entry.  Returns ({key: [B, n_e]},
    same_set [B]) with the entries (i, j), i <= j, in row-major order."""
    B = c['ubar'].shape[0]
    same = np.ones(B, dtype=bool)
    set0 = _snap(base['U'], spec)[0] if spec.boxed else None
    out = {}
    for key in KEYS:
        W = np.asarray(getattr(spec, NAMES[key]), dtype=np.float64)
        n = W.shape[0]
        cols = []
        for i in range(n):
            for j in range(i, n):
                h = REL_STEP * np.sqrt(W[i, i] * W[j, j])
                D = np.zeros((n, n))
                D[i, j] += 1.0
                D[j, i] += 1.0
                L = []
                for sgn in (1.0, -1.0):
                    sp = dataclasses.replace(spec, **{NAMES[key]: W + sgn * h * D})
                    o = mpc_solve(c['x0'], c['xref'], c['uref'], sp, mode='iterate', xbar=c['xbar'], ubar=c['ubar'])
                    L.append(np.einsum('bki,bki->b', c['gX'], o['X']) + np.einsum('bki,bki->b', c['gU'], o['U']))
                    same &= o['status'] == 0
                    if spec.boxed:
                        same &= (_snap(o['U'], spec)[0] == set0).all(axis=(1, 2)) & ~o['fallback']
                cols.append((L[0] - L[1]) / (2.0 * h))
        out[key] = np.stack(cols, axis=1)
    return out, same


def _predicted(r):
    """<g, D> of every independent entry: g_ij + g_ji, in _fd's order."""
    out = {}
    for key in KEYS:
        g = r[key]
        iu = np.triu_indices(g.shape[-1])
        out[key] = g[:, iu[0], iu[1]] + g[:, iu[1], iu[0]]
    return out


def _compare(fd, pred, count, tag):
    allmax = np.max([np.abs(pred[k]).max(axis=1) for k in KEYS], axis=0)
    worst = {}
    for k in KEYS:
        d = np.abs(fd[k] - pred[k]).max(axis=1)
        own = d / np.abs(pred[k]).max(axis=1)
        worst[k] = own[count].max()
        print(f'{tag} {k}: worst difference {worst[k]:.2e} of the output\'s largest entry, '
              f'{(d / allmax)[count].max():.2e} of the instance\'s largest entry (|entry| max {np.abs(pred[k]).max():.3g})')
    for k in KEYS:
        assert worst[k] <= BOUND, (tag, k, worst[k])


@pytest.mark.parametrize('weights', ['default', 'dense'])
def test_reference_matches_finite_differences_unconstrained(weights):
    B, N = 16, 5
    spec = OcpSpec(N=N, **(ac.weights12() if weights == 'dense' else {}))
    c = vjp_case(B, N, spec)
    base = mpc_solve(c['x0'], c['xref'], c['uref'], spec, mode='iterate', xbar=c['xbar'], ubar=c['ubar'])
    assert np.all(base['status'] == 0)
    r = vjp_weights_ref(c['xbar'], c['ubar'], base['X'], base['U'], c['xref'], c['uref'], c['gX'], c['gU'], spec)
    for k in KEYS:
        assert np.array_equal(r[k], np.swapaxes(r[k], 1, 2))
    fd, ok = _fd(c, spec, base)
    assert ok.all()
    _compare(fd, _predicted(r), ok, f'unconstrained {weights} B={B} N={N}')


def test_reference_matches_finite_differences_input_box():
    B, N = 16, 8
    spec = OcpSpec(N=N, lbu=np.full(4, 5.0), ubu=np.full(4, 40.0))
    c = vjp_case(B, N, spec)
    base = mpc_solve(c['x0'], c['xref'], c['uref'], spec, mode='iterate', xbar=c['xbar'], ubar=c['ubar'])
    assert np.all(base['status'] == 0) and not base['fallback'].any()
    fixed, Us = _snap(base['U'], spec)
    r = vjp_weights_ref(c['xbar'], c['ubar'], base['X'], Us, c['xref'], c['uref'], c['gX'], c['gU'], spec)
    assert np.array_equal(r['fixed'], fixed)
    fd, same = _fd(c, spec, base)
    clamped = fixed.any(axis=(1, 2))
    print(f'box B={B} N={N}: {same.sum()} instances count, {(same & clamped).sum()} of them with a clamped '
          f'component ({fixed.sum()} clamped components)')
    assert same.sum() >= 14 and (same & clamped).sum() >= 8
    _compare(fd, _predicted(r), same, f'box B={B} N={N}')
    # the box matters: a reference (or a kernel) that ignores it is far off
    free = vjp_weights_ref(c['xbar'], c['ubar'], base['X'], Us, c['xref'], c['uref'], c['gX'], c['gU'], spec,
                           boxed=False)
    for k in KEYS:
        dif = np.abs(free[k] - r[k]).max(axis=(1, 2)) / np.abs(r[k]).max(axis=(1, 2))
        print(f'box against unconstrained reference, {k}, per instance:', np.array2string(dif, precision=2))
        assert (dif > 0.1).sum() >= 8


def test_entry_points_are_declared_and_bound():
    from mpc_blaster_amd import _lib
    txt = open(os.path.join(REPO, 'include', 'mpcb.h')).read()
    declared = set(re.findall(r'\b(mpcb_[a-z_]+)\s*\(', txt))
    for name in ('mpcb_solve_vjp_w', 'mpcb_set_weights'):
        assert name in declared and name in _lib.EXPORTS
    assert set(_lib.EXPORTS) == declared
    assert re.search(r'#define\s+MPCB_ABI_VERSION\s+5\b', txt) and _lib.ABI_VERSION == 5
