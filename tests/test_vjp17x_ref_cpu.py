"""tests/vjp17x_ref.py (the NumPy references of mpcb_solve_vjp17_sx, the 17/6 product with active
state rows) against each other and against central differences of the oracle's state-box solve;
the input conditions the GPU tests rely on; the bound ``SX_BOUND`` they use; the declaration of
the entry point.  No GPU.

These certify the yardstick of tests/test_gpu_vjp17x.py, not the device.  Metric: the project's,
per instance and output |a - b|_inf / max(|b|_inf, 1).

``SX_BOUND``.  The device runs the recursion that ``al_x`` models, with a penalty of 1e8 on the
active rows, and is compared with ``dense_x``, which has no penalty.  The bound is therefore the
model's own error against the dense solve, 10 x its worst value over the short cases (the margin
covers the device's different summation order), never below 1e-9, the fp64 bound of the other
products.  Measured: worst 2.3e-8 (the synthetic (7, 17) case), so SX_BOUND = 2.3e-7; the test
prints both and holds vjp17x_ref.SX_BOUND to them.

Central differences.  The polished state-box solve is piecewise affine in (x0, xref, uref), so a
central difference is exact up to rounding while both masks hold; the polish leaves its rows
within 1e-10 of their bounds, which the difference divides by 2 h = 2e-4: 1e-6 is the bound, as
in tests/test_vjp17_ref_cpu.py.  h = 1e-4 keeps the masks of all five instances of the (5, 12)
draw (1e-3 loses three), measured 7e-12 for ``dense_x`` and 2e-8 for ``al_x``.
"""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vjp17_ref as vr    # noqa: E402
import vjp17x_ref as xr   # noqa: E402

from oracle.full import FullSpec, mpc_solve17   # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_H, fd_direction = xr.FD_H, xr.fd_direction   # tests/test_gpu_vjp17x.py takes the same step and direction


def _both(c, fixed, fixed_x, spec):
    args = (c['xbar'], c['ubar'], c['p'], fixed, fixed_x, c['gX'], c['gU'], spec)
    return xr.dense_x(*args), xr.al_x(*args)


def _err(a, d):
    return np.max([vr.relerr(a[k], d[k]) for k in xr.KEYS], axis=0)


def test_constants_are_the_header_s():
    txt = open(os.path.join(REPO, 'mpc_blaster_amd', 'csrc', 'mpcb_full.h')).read()
    m = re.search(r'#define MPCB_SX17_RHO ([0-9.e+-]+)\n#endif\nconstexpr double SX17_RHO = MPCB_SX17_RHO, '
                  r'SX17_EQ = ([0-9.e+-]+);\s*constexpr int SX17_ITERS = (\d+);', txt)
    assert m, 'SX17_* not found in mpcb_full.h'
    assert (float(m.group(1)), float(m.group(2)), int(m.group(3))) == (xr.SX17_RHO, xr.SX17_EQ, xr.SX17_ITERS)
    assert (xr.SX17_EQ, xr.SX17_ITERS) == (1e-10, 12)


def test_recursion_matches_dense_kkt_and_fixes_the_bound():
    worst = 0.0
    # synthetic masks on the unboxed draws
    rows = {(5, 3): (0, 3), (7, 17): (7, 13)}
    for (B, N), (lo, hi) in rows.items():
        c, fixed, fixed_x = xr.synth_case(B, N)
        n = fixed_x.sum(axis=(1, 2))
        assert n.min() == lo and n.max() == hi, n
        assert not fixed_x[:, 0].any() and not fixed_x[:, N].any()
        d, a = _both(c, fixed, fixed_x, FullSpec(N=N))
        assert (a['status'] == 0).all() and a['passes'].max() <= 5
        e = _err(a, d)
        print(f'synthetic B={B} N={N}: rows {n}, passes {a["passes"]}, al_x vs dense_x {e.max():.2e}')
        worst = max(worst, e.max())
        if N == 3:   # the instance without rows is the plain product
            b0 = int(np.flatnonzero(n == 0)[0])
            plain = vr.vjp17_ref(c['xbar'], c['ubar'], c['p'], fixed, c['gX'], c['gU'], FullSpec(N=N))
            for k in xr.KEYS:
                assert vr.relerr(d[k][b0:b0 + 1], plain[k][b0:b0 + 1]).max() <= 1e-11, k
                assert vr.relerr(a[k][b0:b0 + 1], plain[k][b0:b0 + 1]).max() <= 1e-11, k
            assert a['passes'][b0] == 1
    n60 = xr.synth_case(3, 60)[2].sum(axis=(1, 2))
    assert n60.min() == 17 and n60.max() == 26, n60
    # end to end: the oracle's masks on the state-box draws
    spec, c = xr.sbox_case(5, 12)
    assert (c['o']['status'] == 0).all()
    n = c['fixed_x'].sum(axis=(1, 2))
    assert n.min() == 28 and n.max() == 32, n
    d, a = _both(c, c['fixed'], c['fixed_x'], spec)
    assert (a['status'] == 0).all()
    e = _err(a, d)
    print(f'end to end B=5 N=12: rows {n}, passes {a["passes"]}, al_x vs dense_x {e.max():.2e}')
    worst = max(worst, e.max())
    plain = vr.vjp17_ref(c['xbar'], c['ubar'], c['p'], c['fixed'], c['gX'], c['gU'], spec)
    assert (_err(plain, d) > 0.5).all()   # the product that ignores the state rows is simply wrong
    # the stalling instance: a nearly dependent active set, at any penalty
    spec, c = xr.sbox_case(8, 20)
    assert (c['o']['status'] == 0).all()
    n = c['fixed_x'].sum(axis=(1, 2))
    assert n.min() == 38 and n.max() == 57, n
    d, a = _both(c, c['fixed'], c['fixed_x'], spec)
    assert list(a['status']) == [2] + [0] * 7 and a['passes'][0] == xr.SX17_ITERS
    e = _err(a, d)
    print(f'end to end B=8 N=20: rows {n}, passes {a["passes"]}, eq[0] {a["eq"][0]:.2e}, al_x vs dense_x '
          f'{np.array2string(e, precision=2)}')
    worst = max(worst, e[1:].max())
    bound = max(1e-9, 10.0 * worst)
    print(f'worst al_x vs dense_x over the short cases {worst:.2e}: SX_BOUND = {bound:.2e} '
          f'(vjp17x_ref.SX_BOUND {xr.SX_BOUND:.2e})')
    assert 0.5 * xr.SX_BOUND <= bound <= xr.SX_BOUND


def _masks(o, c, spec):
    return ((vr.active_mask(o['U'], spec)[0] == c['fixed']).all(axis=(1, 2)) &
            (xr.state_mask(o['X'], c['lbx'], c['ubx'])[0] == c['fixed_x']).all(axis=(1, 2)) & (o['status'] == 0))


def test_references_match_central_differences_of_the_state_box_solve():
    B, N = 5, 12
    spec, c = xr.sbox_case(B, N)
    d0, dr, du = fd_direction(B, N)
    d, a = _both(c, c['fixed'], c['fixed_x'], spec)
    for with_uref in (True, False):   # (False: the direction of the torch-layer test on the GPU)
        du_ = du if with_uref else np.zeros_like(du)
        L, stable = [], np.ones(B, dtype=bool)
        for sg in (1.0, -1.0):
            o = mpc_solve17(c['x0'] + sg * FD_H * d0, c['xref'] + sg * FD_H * dr, c['uref'] + sg * FD_H * du_, spec,
                            c['p'], mode='iterate', xbar=c['xbar'], ubar=c['ubar'])
            L.append(np.einsum('bki,bki->b', c['gX'], o['X']) + np.einsum('bki,bki->b', c['gU'], o['U']))
            stable &= _masks(o, c, spec)
        assert stable.sum() >= 3, stable
        fd = (L[0] - L[1]) / (2.0 * FD_H)
        for name, r, tol in (('dense_x', d, 1e-6), ('al_x', a, 1e-6 + xr.SX_BOUND)):
            lin = (np.einsum('bi,bi->b', r['gx0'], d0) + np.einsum('bki,bki->b', r['gxref'], dr) +
                   np.einsum('bki,bki->b', r['guref'], du_))
            rel = np.abs(fd - lin) / np.maximum(np.abs(lin), 1.0)
            print(f'{name} vs central differences (uref moved: {with_uref}), stable {stable.astype(int)}: '
                  f'{np.array2string(rel, precision=2)}')
            assert rel[stable].max() <= tol, (name, rel)


def test_closed_loop_case_of_the_gpu_test():
    """The two-step state-box loop of tests/test_gpu_vjp17x.py: every solve has status 0 and active state
    rows, and the chained reference gradient agrees with a central difference of the loop along
    (x0, xref) while the masks hold (h = 1e-5; the bound of the other difference tests, 1e-6)."""
    L = xr.loop_case()
    c, spec, w = L['c'], L['spec'], L['w']
    B, N = xr.LOOP_B, xr.LOOP_N
    for st in L['steps']:
        assert (st['status'] == 0).all() and st['fixed_x'].any(axis=(1, 2)).all()
    rng = np.random.default_rng(xr.FD_SEED)
    d0, dr = rng.standard_normal((B, 17)), rng.standard_normal((B, N + 1, 17))
    h = 1e-5
    assert L['ok'].tolist() == [[True, False, True], [True, True, True]]   # (vjp17x_ref.loop_case)
    Ls, stable = [], L['ok'].all(axis=0)
    for sg in (1.0, -1.0):
        X, _, steps = xr.loop_ref(c, spec, x0=c['x0'] + sg * h * d0, xref=c['xref'] + sg * h * dr)
        Ls.append((w * X).sum(axis=(1, 2)))
        for a, b in zip(steps, L['steps']):
            stable &= ((a['fixed'] == b['fixed']).all(axis=(1, 2)) & (a['fixed_x'] == b['fixed_x']).all(axis=(1, 2)) &
                       (a['status'] == 0))
    fd = (Ls[0] - Ls[1]) / (2.0 * h)
    lin = np.einsum('bi,bi->b', L['grad']['x0'], d0) + np.einsum('bki,bki->b', L['grad']['xref'], dr)
    rel = np.abs(fd - lin) / np.maximum(np.abs(lin), 1.0)
    print(f'closed loop: rows per step {[s["fixed_x"].sum(axis=(1, 2)) for s in L["steps"]]}, stable '
          f'{stable.astype(int)}, chained reference vs central differences {np.array2string(rel, precision=2)}')
    assert stable.sum() >= 2 and rel[stable].max() <= 1e-6


def test_entry_point_is_declared_and_bound():
    from mpc_blaster_amd import _lib
    txt = open(os.path.join(REPO, 'include', 'mpcb.h')).read()
    assert re.search(r'\bint\s+mpcb_solve_vjp17_sx\s*\(', txt)
    assert 'mpcb_solve_vjp17_sx' in _lib.EXPORTS_17 and 'mpcb_solve_vjp17_sx' not in _lib.EXPORTS
    assert re.search(r'#define\s+MPCB_ABI_VERSION\s+5\b', txt) and _lib.ABI_VERSION == 5
    assert 'the state box is not covered' not in open(os.path.join(REPO, 'README.md')).read()
