"""tests/pw17_ref.py (the NumPy references of mpcb_solve_iterate_pw17 and mpcb_solve_vjp_pw17)
against the batched oracle and against central finite differences in the weights, and the
declaration of the two entry points.  No GPU.

These certify the yardstick of tests/test_gpu_pw17.py, not the device.  Metric: the project's,
|a - b|_inf / max(|b|_inf, 1), per instance and per weight matrix.

The weight check.  L = <gX, X> + <gU, U> of the unboxed step is a smooth (rational) function of an
instance's weights.  One diagonal entry and one symmetric off-diagonal pair of each of Q, R, QN are
moved by +-h, h = 1e-4 of the entry's own scale (sqrt(W_ii W_jj) for a pair), and the central
difference is compared with the reference's gQ, gR, gQN: dL = gW_ii h for a diagonal entry,
(gW_ij + gW_ji) h for a pair.  The bounds are those of tests/test_vjp17_ref_cpu.py for its central
differences of the same step: 1e-8 for the state weights (its gx0 / gxref bound), 1e-6 for R (its
guref bound: the swivel-rate weights are 1e-5, which the difference divides by).
"""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pw17_ref as pr   # noqa: E402
import vjp17_ref as vr  # noqa: E402

from oracle.full import FullSpec, mpc_solve17   # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_solve_helper_equals_batched_oracle_at_the_specs_weights():
    B, N = 3, 4
    spec = FullSpec(N=N)
    c = vr.vjp17_case(B, N, spec)
    o = mpc_solve17(c['x0'], c['xref'], c['uref'], spec, c['p'], mode='iterate', xbar=c['xbar'], ubar=c['ubar'])
    tile = lambda M: np.tile(np.asarray(M, dtype=np.float64)[None], (B, 1, 1))   # noqa: E731
    for kw in (dict(), dict(Q=tile(spec.Q), R=tile(spec.R), QN=tile(spec.QN)), dict(R=tile(spec.R)[:1])):
        r = pr.pw17_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, c['p'], **kw)
        assert (r['status'] == o['status']).all() and (r['status'] == 0).all()
        for k in ('u0', 'X', 'U'):
            assert vr.relerr(r[k], o[k]).max() <= 1e-13, k


def test_weights_are_spd_congruences_with_the_specs_terminal_default():
    spec = FullSpec(N=4)
    Q, R, QN = pr.pw17_weights(5, spec, sigma=0.7, seed=3)
    assert Q.shape == (5, 17, 17) and R.shape == (5, 6, 6) and QN.shape == (5, 17, 17)
    for W, W0 in ((Q, spec.Q), (R, spec.R), (QN, 10.0 * np.asarray(spec.Q))):
        assert (W == W.transpose(0, 2, 1)).all() and (np.linalg.eigvalsh(W) > 0).all()
        d = np.sqrt(np.diagonal(W, axis1=1, axis2=2) / np.diag(W0))   # W_b = W0 o (e e^T)
        assert np.allclose(W, np.asarray(W0) * d[:, :, None] * d[:, None, :], rtol=1e-13, atol=0)
        assert d.std() > 0.2   # sigma = 0.7: the instances differ


def test_weight_gradients_match_finite_differences():
    B, N = 3, 4
    spec = FullSpec(N=N)
    c = vr.vjp17_case(B, N, spec)
    W = dict(zip(pr.WNAMES, pr.pw17_weights(B, spec, sigma=0.7, seed=5)))
    solve = lambda w: pr.pw17_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, c['p'], **w)   # noqa: E731
    base = solve(W)
    assert (base['status'] == 0).all()
    g = pr.pw17_vjp_ref(c['xbar'], c['ubar'], c['p'], None, c['gX'], c['gU'], spec, X=base['X'], U=base['U'],
                        xref=c['xref'], uref=c['uref'], **W)
    loss = lambda o: np.einsum('bki,bki->b', c['gX'], o['X']) + np.einsum('bki,bki->b', c['gU'], o['U'])   # noqa: E731
    bounds = dict(Q=1e-8, R=1e-6, QN=1e-8)
    probes = dict(Q=((3, 3), (0, 4)), R=((1, 1), (0, 5)), QN=((7, 7), (2, 9)))
    for name, key in zip(pr.WNAMES, vr.WKEYS):
        assert (g[key] == g[key].transpose(0, 2, 1)).all()
        for i, j in probes[name]:
            h = 1e-4 * np.sqrt(W[name][:, i, i] * W[name][:, j, j])   # per instance
            L = []
            for sgn in (1.0, -1.0):
                Wp = {k: v.copy() for k, v in W.items()}
                Wp[name][:, i, j] += sgn * h
                if i != j:
                    Wp[name][:, j, i] += sgn * h
                o = solve(Wp)
                assert (o['status'] == 0).all()
                L.append(loss(o))
            fd = (L[0] - L[1]) / (2.0 * h)
            an = g[key][:, i, j] if i == j else g[key][:, i, j] + g[key][:, j, i]
            err = np.abs(fd - an) / np.maximum(np.abs(g[key]).reshape(B, -1).max(axis=1), 1.0)
            print(f'{key}[{i},{j}]: central difference {np.array2string(fd, precision=6)} reference '
                  f'{np.array2string(an, precision=6)} rel err {np.array2string(err, precision=2)}')
            assert err.max() <= bounds[name], (key, i, j, err)


def test_entry_points_are_declared_and_bound():
    from mpc_blaster_amd import _lib
    txt = open(os.path.join(REPO, 'include', 'mpcb.h')).read()
    for name in ('mpcb_solve_iterate_pw17', 'mpcb_solve_vjp_pw17'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', txt)
        assert name in _lib.EXPORTS_17 and name not in _lib.EXPORTS
    assert re.search(r'#define\s+MPCB_ABI_VERSION\s+5\b', txt) and _lib.ABI_VERSION == 5
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in _lib.EXPORTS_17)
    # the six weight arguments on top of mpcb_solve_iterate (less its wind pair) and mpcb_solve_vjp17
    assert len(lib.mpcb_solve_iterate_pw17.argtypes) == len(lib.mpcb_solve_iterate.argtypes) - 2 + 6
    assert len(lib.mpcb_solve_vjp_pw17.argtypes) == len(lib.mpcb_solve_vjp17.argtypes) + 6
