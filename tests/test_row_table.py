"""Weights::rowt, the lane-ordered table of the row rollout's lane constants that mpcb_create fills
on the host (mpcb_capi.hip fill_row_table), read back through mpcb_debug_row_table and checked
entry by entry against a NumPy restatement of the per-lane formulas the kernel used to evaluate in
every wave (mpcb_row.h row_body before the table).  Host only: no device is touched.

Tolerance: the selectors, copies and zeros are exact.  The sums (G, Lm, Ju, kd) are three-term
fp64 dot products that the library forms with fused multiply-adds and NumPy with separate
roundings, so they may differ by a few units in the last place of their largest term: 8 eps of
sum |terms|.  The fp32 table is the same arithmetic in float, checked against the fp64
restatement at 8 float eps.
"""
import ctypes

import numpy as np
import pytest

from mpc_blaster_amd import MPCConfig, _lib

NZ, NX = 16, 12
# slots of a lane's record (mpcb_kernels.h ROWT_*)
G3, LM, GRAV, DSL, JU, KD, PAD, JROW, G0, W = 0, 3, 7, 8, 9, 12, 15, 16, 19, 22


def _general_j():
    J = np.diag([0.50781, 0.47314, 0.72975])
    J[0, 1] = J[1, 0] = 0.01
    J[1, 2] = J[2, 1] = -0.004
    return J


def _table(cfg):
    lib = _lib.load()
    f = lib.mpcb_debug_row_table
    f.argtypes = [ctypes.POINTER(_lib.MpcbConfig), ctypes.c_void_p]
    f.restype = ctypes.c_int
    out = np.full(NZ * W, np.nan)
    c = cfg.to_c()
    _lib.check(f(ctypes.byref(c), out.ctypes.data))
    return out.reshape(NZ, W)


def _reference(cfg):
    """(value, magnitude) per slot: magnitude = sum of |terms|, 0 where the entry is exact."""
    J = np.asarray(cfg.J, dtype=np.float64)
    Ji = np.linalg.inv(J)
    minv = 1.0 / cfg.mass
    # (w x Jw)_i = sum_jl B_i[j][l] w_j w_l, B_i[j][l] = sum_m eps_ijm J_ml, over the products
    # p = (w0 w0, w1 w1, w2 w2, w0 w1, w0 w2, w1 w2)
    coef = np.zeros((3, 6))
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        B = np.zeros((3, 3))
        B[i1, :] += J[i2, :]
        B[i2, :] -= J[i1, :]
        coef[i] = [B[0, 0], B[1, 1], B[2, 2], B[0, 1] + B[1, 0], B[0, 2] + B[2, 0], B[1, 2] + B[2, 1]]
    lx, ly, c = cfg.lx, cfg.ly, cfg.c
    mix = np.array([[-ly, ly, -ly, ly], [-lx, lx, lx, -lx], [-c, -c, c, c]])
    val = np.zeros((NZ, W))
    mag = np.zeros((NZ, W))
    for t in range(NZ):
        r = t - 9 if 9 <= t < 12 else -1
        jir = Ji[r] if r >= 0 else np.zeros(3)
        g = -(jir @ coef)
        gm = np.abs(jir) @ np.abs(coef)
        val[t, G0:G0 + 3], mag[t, G0:G0 + 3] = g[:3], gm[:3]
        val[t, G3:G3 + 3], mag[t, G3:G3 + 3] = g[3:], gm[3:]
        val[t, LM:LM + 4], mag[t, LM:LM + 4] = jir @ mix, np.abs(jir) @ np.abs(mix)
        val[t, JROW:JROW + 3] = J[r if r >= 0 else 0]
        val[t, GRAV] = cfg.g if t == 8 else 0.0
        m = t - NX if t >= NX else -1
        val[t, DSL] = minv if m >= 0 else 0.0
        if m >= 0:
            val[t, JU:JU + 3], mag[t, JU:JU + 3] = Ji @ mix[:, m], np.abs(Ji) @ np.abs(mix[:, m])
        val[t, KD:KD + 3] = [-Ji[0, 0] * (J[2, 2] - J[1, 1]), -Ji[1, 1] * (J[0, 0] - J[2, 2]),
                             -Ji[2, 2] * (J[1, 1] - J[0, 0])]
        mag[t, KD:KD + 3] = [abs(Ji[0, 0]) * (J[2, 2] + J[1, 1]), abs(Ji[1, 1]) * (J[0, 0] + J[2, 2]),
                             abs(Ji[2, 2]) * (J[1, 1] + J[0, 0])]
    return val, mag


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('inertia', ['diagonal', 'general'])
def test_row_table_matches_lane_formulas(inertia, dtype):
    kw = {} if inertia == 'diagonal' else {'J': _general_j()}
    cfg = MPCConfig(N=20, dtype=dtype, mass=8.7, g=9.80665, **kw)
    tab = _table(cfg)
    val, mag = _reference(cfg)
    assert np.isfinite(tab).all()
    eps = np.finfo(np.float64 if dtype == 'f64' else np.float32).eps
    # Jinv itself is inverted in fp64 by both sides with different formulas: a few eps of its entries
    tol = 8 * eps * mag + (4 * eps * np.abs(val) if dtype == 'f64' else 0)
    exact = mag == 0
    if dtype == 'f32':   # the exact entries are the fp64 values rounded once
        val = np.where(exact, val.astype(np.float32).astype(np.float64), val)
    # copies, selectors and zeros: exact (1/m is one division on both sides)
    assert np.array_equal(tab[exact], val[exact])
    err = np.abs(tab - val)
    worst = np.unravel_index(np.argmax(err - tol), err.shape)
    print(f'{inertia} {dtype}: max |err| {err.max():.3e}, worst slot {worst} err {err[worst]:.3e} tol {tol[worst]:.3e}')
    assert (err[~exact] <= tol[~exact]).all()
    assert (tab[:, PAD] == 0).all()


def test_row_table_structure_diagonal_inertia():
    """What the diagonal-inertia kernel relies on: state lanes carry no input direction, only lanes
    9..11 a gyroscopic form and a mixer row, and the form of a diagonal J has one product per rate."""
    tab = _table(MPCConfig(N=20))
    assert (tab[:9, G3:G3 + 3] == 0).all() and (tab[12:, G3:G3 + 3] == 0).all()
    assert (tab[:9, LM:LM + 4] == 0).all() and (tab[12:, LM:LM + 4] == 0).all()
    assert (tab[:, G0:G0 + 3] == 0).all()                 # no w_i^2 terms for a diagonal J
    # rate 0 <- w1 w2 (slot G3 + 2), rate 1 <- w0 w2 (G3 + 1), rate 2 <- w0 w1 (G3 + 0)
    for lane, slot in ((9, G3 + 2), (10, G3 + 1), (11, G3)):
        row = tab[lane, G3:G3 + 3]
        assert row[slot - G3] != 0 and np.count_nonzero(row) == 1
    assert (tab[:NX, DSL] == 0).all() and (tab[NX:, DSL] == 1.0 / 9.0).all()
    assert (tab[:NX, JU:JU + 3] == 0).all()
    assert (tab[:, GRAV] == np.where(np.arange(NZ) == 8, 9.81, 0.0)).all()
    # kd does not depend on the lane
    assert (tab[:, KD:KD + 3] == tab[0, KD:KD + 3]).all()
