"""tests/pw_ref.py (the NumPy references of mpcb_solve_iterate_pw and mpcb_solve_vjp_pw) against the
batched oracle and against central finite differences of its own solve, and the declaration of
the two entry points.  No GPU.

Finite differences: the method and bound of tests/test_vjp_weights_ref_cpu.py.  L = <gX, X> + <gU, U>
of ONE instance; for the entry (i, j), i <= j, of one of its matrices W the probe is W +- h D with
D = E_ij + E_ji and h = 1e-4 sqrt(W_ii W_jj), and the reference predicts (L+ - L-) / 2h = g_ij + g_ji.
Bound: 1e-6 of the output's largest predicted entry.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alt_config as ac   # noqa: E402
from pw_ref import no_early_handover, pw_solve_ref, pw_vjp_ref, pw_weights   # noqa: E402
from test_vjp_ref_cpu import _snap   # noqa: E402
from vjp_ref import vjp_case   # noqa: E402

from oracle.ocp import OcpSpec, mpc_solve   # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LB, UB = np.full(4, 5.0), np.full(4, 40.0)
KEYS = ('gQ', 'gR', 'gQN')
BOUND = 1e-6
REL_STEP = 1e-4


def test_weight_draw_is_spd_and_differs():
    spec = OcpSpec(N=3, **ac.weights12())
    Q, R, QN = pw_weights(5, spec)
    for W, W0 in ((Q, spec.Q), (R, spec.R), (QN, spec.QN)):
        assert np.array_equal(W, np.swapaxes(W, 1, 2))
        assert np.linalg.eigvalsh(W).min() > 0
        assert np.abs(W - np.asarray(W0)[None]).max() > 1e-2 and np.abs(W[0] - W[1]).max() > 1e-2
    a, b = pw_weights(5, spec), pw_weights(7, spec)
    assert all(np.array_equal(x, y[:5]) for x, y in zip(a, b))   # instance b's draw does not depend on B


@pytest.mark.parametrize('box', [False, True])
def test_equal_weights_reproduce_the_batched_oracle(box):
    B, N = 6, 5
    spec = OcpSpec(N=N, lbu=LB if box else None, ubu=UB if box else None)
    c = vjp_case(B, N, spec, 'sine', True)
    with no_early_handover():
        o = mpc_solve(c['x0'], c['xref'], c['uref'], spec, wind=c['wind'], mode='iterate', xbar=c['xbar'],
                      ubar=c['ubar'])
    tile = lambda W: np.tile(np.asarray(W)[None], (B, 1, 1))   # noqa: E731
    r = pw_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, tile(spec.Q), tile(spec.R),
                     tile(spec.QN), c['wind'])
    none = pw_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, wind=c['wind'])
    assert not o['fallback'].any() and not r['fallback'].any()
    for k in ('u0', 'X', 'U'):
        assert np.abs(r[k] - o[k]).max() <= 1e-12 * max(1.0, np.abs(o[k]).max()), k
        assert np.array_equal(r[k], none[k]), k
    assert np.array_equal(r['status'], o['status']) and np.array_equal(r['iters'], o['iters'])
    # and per-instance weights do change the solution
    Q, R, QN = pw_weights(B, spec)
    p = pw_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, Q, R, QN, c['wind'])
    assert np.abs(p['U'] - o['U']).reshape(B, -1).max(axis=1).min() > 1e-3


def _fd_one(c, spec, W3, b):
    """Central differences of instance b's L over every independent entry of its three matrices.
    Returns ({key: [n_e]}, same_set)."""
    one = {k: (None if v is None else v[b:b + 1]) for k, v in c.items()}
    Wb = [W[b:b + 1] for W in W3]

    def solve(Wl):
        return pw_solve_ref(one['x0'], one['xref'], one['uref'], one['xbar'], one['ubar'], spec, *Wl, one['wind'])

    base = solve(Wb)
    set0 = _snap(base['U'], spec)[0] if spec.boxed else None
    same = bool(base['status'][0] == 0 and not base['fallback'][0])
    out = {}
    for idx, key in enumerate(KEYS):
        W = Wb[idx][0]
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
                    Wl = list(Wb)
                    Wl[idx] = (W + sgn * h * D)[None]
                    o = solve(Wl)
                    L.append(np.sum(one['gX'] * o['X']) + np.sum(one['gU'] * o['U']))
                    same &= bool(o['status'][0] == 0 and not o['fallback'][0])
                    if spec.boxed:
                        same &= bool((_snap(o['U'], spec)[0] == set0).all())
                cols.append((L[0] - L[1]) / (2.0 * h))
        out[key] = np.array(cols)
    return out, same, base


@pytest.mark.parametrize('weights,box,b', [('default', False, 1), ('dense', False, 2), ('default', True, 1)])
def test_gradients_match_finite_differences_of_the_solve(weights, box, b):
    B, N = 3, 8 if box else 5
    spec = OcpSpec(N=N, lbu=LB if box else None, ubu=UB if box else None,
                   **(ac.weights12() if weights == 'dense' else {}))
    c = vjp_case(B, N, spec)
    W3 = pw_weights(B, spec)
    fd, same, base = _fd_one(c, spec, W3, b)
    assert same
    Ub = _snap(base['U'], spec)[1] if box else base['U']
    if box:
        assert _snap(base['U'], spec)[0].any()   # the instance does have clamped components
    # the reference on the whole batch (the other instances solve with their own matrices)
    full = pw_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, *W3)
    assert np.array_equal(full['U'][b], base['U'][0])
    X, U = full['X'].copy(), (_snap(full['U'], spec)[1] if box else full['U'].copy())
    assert np.array_equal(U[b], Ub[0])
    r = pw_vjp_ref(c['xbar'], c['ubar'], X, U, c['xref'], c['uref'], c['gX'], c['gU'], spec, *W3)
    for k in KEYS:
        g = r[k][b]
        assert np.array_equal(g, g.T)
        iu = np.triu_indices(g.shape[0])
        pred = g[iu] + g.T[iu]
        d = np.abs(fd[k] - pred).max() / np.abs(pred).max()
        print(f'{weights} box={box} instance {b} {k}: worst difference {d:.2e} of the output\'s largest entry '
              f'(|entry| max {np.abs(pred).max():.3g})')
        assert d <= BOUND, (k, d)


def test_entry_points_are_declared_and_bound():
    from mpc_blaster_amd import _lib
    txt = open(os.path.join(REPO, 'include', 'mpcb.h')).read()
    declared = set(re.findall(r'\b(mpcb_[a-z_]+)\s*\(', txt))
    for name in ('mpcb_solve_iterate_pw', 'mpcb_solve_vjp_pw'):
        assert name in declared and name in _lib.EXPORTS
        assert re.search(r'\bint\s+' + name + r'\s*\(', txt)
    assert set(_lib.EXPORTS) == declared
    assert re.search(r'#define\s+MPCB_ABI_VERSION\s+5\b', txt) and _lib.ABI_VERSION == 5
    lib = _lib.load()
    assert len(lib.mpcb_solve_iterate_pw.argtypes) == 23 and len(lib.mpcb_solve_vjp_pw.argtypes) == 28
    # the header says what the C ABI cannot check, and what the call leaves alone
    doc = txt[:txt.index('int mpcb_solve_iterate_pw(')]
    doc = doc[doc.rindex('/*'):]
    assert 'symmetric' in doc and 'mpcb_qp_stats is not updated' in doc and 'Out of scope' in doc
