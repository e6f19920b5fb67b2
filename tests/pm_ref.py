"""NumPy references of mpcb_sim_step_pm, mpcb_solve_iterate_pm and mpcb_solve_gains_pm
(include/mpcb.h): the plant step, the RTI step and its feedback gains with a vehicle per instance;
a helper, not a test.

Each loops over the instances and calls the project's reference on one instance with that
instance's ``oracle.model.Params`` (and, for the solve, weights) in the spec:
``oracle.rk4.rk4_step`` over ``oracle.model.f12``, ``oracle.ocp.mpc_solve(mode='iterate')`` under
tests/pw_ref.py ``no_early_handover`` (the entry point's input box is the plain active set), and
tests/gains_ref.py ``gains_ref``.  Gravity stays the spec's.

A vehicle is the record of the C ABI, MPCB_MODEL_REC = 14 values:
  [0] mass  [1] lx  [2] ly  [3] c  [4] t_blast  [5..13] J row-major
``models`` arguments are [B|1, 14] arrays of such records.
"""
import dataclasses

import numpy as np

from oracle.model import f12
from oracle.ocp import mpc_solve
from oracle.rk4 import rk4_step

from gains_ref import gains_ref
from pw_ref import _row, _spec_b, no_early_handover

MODEL_REC = 14
SKEYS = ('u0', 'X', 'U', 'status', 'iters', 'fallback')


def pack_params(P):
    """The record of an ``oracle.model.Params``."""
    return np.concatenate([[P.mass, P.lx, P.ly, P.c, P.t_blast], np.asarray(P.J, dtype=np.float64).reshape(9)])


def params_of(rec, base):
    """``oracle.model.Params`` of a record; gravity from ``base``."""
    rec = np.asarray(rec, dtype=np.float64)
    return dataclasses.replace(base, mass=float(rec[0]), lx=float(rec[1]), ly=float(rec[2]), c=float(rec[3]),
                               t_blast=float(rec[4]), J=rec[5:14].reshape(3, 3).copy())


def pm_models(B, spec, seed=21):
    """[B, 14] test vehicles around the spec's: mass x U(0.8, 1.25); lx, ly, c x U(0.9, 1.1);
    t_blast U(0, 5); J = E J0 E with E = diag(exp(0.2 N(0, 1))) plus a symmetric off-diagonal of at
    most 2% of the smallest diagonal entry: symmetric positive definite and dense."""
    rng = np.random.default_rng(seed)
    P0 = spec.params
    J0 = np.asarray(P0.J, dtype=np.float64)
    out = np.empty((B, MODEL_REC))
    for b in range(B):
        mass = P0.mass * rng.uniform(0.8, 1.25)
        lx, ly, c = (v * rng.uniform(0.9, 1.1) for v in (P0.lx, P0.ly, P0.c))
        tb = rng.uniform(0.0, 5.0)
        e = np.exp(0.2 * rng.standard_normal(3))
        J = J0 * np.outer(e, e)
        off = 0.02 * np.diag(J).min() * rng.uniform(-1.0, 1.0, 3)
        for (i, j), v in zip(((0, 1), (0, 2), (1, 2)), off):
            J[i, j] += v
            J[j, i] += v
        out[b] = np.concatenate([[mass, lx, ly, c, tb], J.reshape(9)])
    return out


def _spec_m(spec, b, models):
    if models is None:
        return spec
    models = np.asarray(models, dtype=np.float64)
    return dataclasses.replace(spec, params=params_of(models[b if models.shape[0] > 1 else 0], spec.params))


def pm_sim_ref(x, u, T, spec, models=None, wind=None):
    """x_out [B, 12]: one RK4 step of length T of instance b's vehicle."""
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    u = np.asarray(u, dtype=np.float64)
    return np.concatenate([rk4_step(x[b:b + 1], u[b:b + 1], T, _spec_m(spec, b, models).params, _row(wind, b, B), f=f12)
                           for b in range(B)])


def pm_solve_ref(x0, xref, uref, xbar, ubar, spec, models=None, Q=None, R=None, QN=None, wind=None):
    """dict(u0, X, U, status, iters, fallback) of the RTI step in which instance b solves with its
    own vehicle and with Q[b], R[b], QN[b] ([B|1, n, n]; None = the spec's)."""
    x0 = np.asarray(x0, dtype=np.float64)
    B = x0.shape[0]
    Q, R, QN = (None if W is None else np.asarray(W, dtype=np.float64) for W in (Q, R, QN))
    outs = []
    with no_early_handover():
        for b in range(B):
            sb = _spec_m(_spec_b(spec, b, Q, R, QN), b, models)
            outs.append(mpc_solve(x0[b:b + 1], _row(xref, b, B), _row(uref, b, B), sb, wind=_row(wind, b, B),
                                  mode='iterate', xbar=_row(xbar, b, B), ubar=_row(ubar, b, B)))
    return {k: np.concatenate([o[k] for o in outs]) for k in SKEYS}


def pm_gains_ref(xbar, ubar, fixed, spec, models=None, wind=None):
    """dict(K [B,N,4,12], P0 [B,12,12], ok [B]): gains_ref instance by instance at that instance's
    vehicle, with the spec's weights."""
    B = np.asarray(ubar).shape[0]
    outs = [gains_ref(_row(xbar, b, B), _row(ubar, b, B), None if fixed is None else np.asarray(fixed)[b:b + 1],
                      _spec_m(spec, b, models), _row(wind, b, B)) for b in range(B)]
    return {k: np.concatenate([o[k] for o in outs]) for k in ('K', 'P0', 'ok')}
