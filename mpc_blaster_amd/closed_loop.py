"""Device-resident closed-loop Monte-Carlo: the receding-horizon loop of
src/scripts/simulation_blaster.py:56-107 for a whole batch, without leaving the GPU.

Per step (one batch launch each): SQP_RTI solve from the persistent iterate (acados keeps the
iterate between ``solve()`` calls and does not shift it; initial iterate = zeros), then the
plant integrator (AcadosSimSolver: one RK4 step of Tsim = Tf/N, JSON ``Tsim``) applies u0*.
"""
from __future__ import annotations

from .api import BatchedMPC


def closed_loop(mpc: BatchedMPC, x0, x_ref, u_ref, nsim: int, wind=None, plant_T=None,
                xbar=None, ubar=None, diagnostics=False, resolve_every: int = 1, feedback: bool = False,
                active_tol=None, weights=None, model=None, plant_model=None, plant_params=None, weights17=None):
    """Returns (X_sim [B, nsim+1, nx], U_sim [B, nsim, nu], status [B] = max over steps).

    ``resolve_every = h > 1`` (h <= N) models a controller slower than the plant: the solve runs
    on the steps i = 0, h, 2h, ... from the persistent iterate and its trajectories (Xp, Up) are
    kept; step i applies ``Up[:, j]``, j = i mod h, and with ``feedback=True`` the RTI feedback law
    ``Up[:, j] + K[:, j] (x - Xp[:, j])`` with the gains of that solve
    (``BatchedMPC.solve_iterate_gains`` at the iterate the solve started from, on the active set of
    its U), clipped to the input box on a handle that has one.  ``active_tol`` is that call's
    active-set tolerance: required with ``feedback`` on an f32 17/6 input-box handle, which has no
    default (checked before the loop starts), optional elsewhere.  With the defaults every step
    solves, as before.

    ``weights``: a dict with any of the keys ``Q``, ``R``, ``QN``, cost weights per instance by the
    shape rule of ``BatchedMPC.solve_iterate`` (2-D [B|1, n] diagonals, 3-D [B|1, n, n] matrices),
    passed to every solve: B candidate weightings run as one closed-loop batch (12/4 model).  Not
    together with ``feedback=True``, whose gains use the handle's weights, nor with
    ``diagnostics``, which evaluates the handle's cost.

    ``weights17``: the same on the 17/6 model (a 12/4 handle raises ``ValueError``): a dict with any of
    ``Q`` [B|1,17] or [B|1,17,17], ``R`` [B|1,6] or [B|1,6,6], ``QN``; every solve of the loop then goes
    through ``BatchedMPC.solve_iterate_pw17`` with the handle's parameters and boxes.  Not together
    with ``feedback=True`` or ``diagnostics``, for the reasons above.

    ``model`` and ``plant_model`` (12/4 model): vehicle records [B|1, 14] as
    ``BatchedMPC.pack_model`` builds them, in two roles.  ``model`` is the controller's belief: it
    goes to every solve and, with ``feedback=True``, to the gains.  ``plant_model`` is the truth:
    it goes to every plant step.  Either may be given alone; the other side then uses the handle's
    vehicle.  ``model`` not together with ``diagnostics``, which evaluates with the handle's model.

    ``plant_params`` (17/6 model; a 12/4 handle raises ``ValueError``): the plant's parameter vectors
    [25] or [B|1, 25] in the layout of ``set_params``.  They go to every plant step
    (``sim_step(params=)``), with ``resolve_every`` / ``feedback`` too; the controller keeps the
    handle's ``set_params``.  The parameter-mismatch Monte Carlo on one handle.

    ``diagnostics=True`` evaluates the new iterate after each solve (``BatchedMPC.evaluate`` with
    that step's x0) and returns a fourth value: a dict of [B, nsim] tensors ``cost``, ``res_eq``,
    ``res_stat`` (without ``res_stat`` on a handle with a state box)."""
    import torch
    h = int(resolve_every)
    wkw = {}
    if weights is not None:
        unknown = set(weights) - {'Q', 'R', 'QN'}
        if unknown:
            raise ValueError(f'weights: unknown keys {sorted(unknown)} (expected Q, R, QN)')
        if feedback:
            raise ValueError('feedback=True uses the gains of the handle\'s weights: not together with weights')
        if diagnostics:
            raise ValueError('diagnostics evaluates the handle\'s cost: not together with weights')
        wkw = {k: v for k, v in weights.items() if v is not None}
    w17 = _weights17_arg(mpc, weights17, wind)
    if w17 is not None:
        if weights is not None:
            raise ValueError('weights covers the 12/4 model, weights17 the 17/6 model: not both')
        if feedback:
            raise ValueError('feedback=True uses the gains of the handle\'s weights: not together with weights17')
        if diagnostics:
            raise ValueError('diagnostics evaluates the handle\'s cost: not together with weights17')
    mkw, pkw = {}, {}
    if model is not None or plant_model is not None:
        if mpc.nx == 17:
            raise ValueError('model / plant_model cover the 12/4 model only (17/6: set_params)')
        if diagnostics and model is not None:
            raise ValueError('diagnostics evaluates with the handle\'s model: not together with model')
        # records on the device once, not at every step (and checked against the batch here)
        B0 = x0.shape[0] if hasattr(x0, 'shape') else len(x0)
        if model is not None:
            mkw = dict(model=mpc._model_arg(model, B0)[0])
        if plant_model is not None:
            pkw = dict(model=mpc._model_arg(plant_model, B0)[0])
    if plant_params is not None:
        B0 = x0.shape[0] if hasattr(x0, 'shape') else len(x0)
        pkw = dict(params=mpc._params_arg(plant_params, B0)[0])   # ValueError on a 12/4 handle
    if h < 1 or h > mpc.cfg.N:
        raise ValueError(f'resolve_every = {resolve_every}: expected 1 <= resolve_every <= N = {mpc.cfg.N}')
    if h > 1 or feedback:
        if diagnostics:
            raise ValueError('diagnostics evaluates every step\'s solve: use resolve_every=1, feedback=False')
        if feedback and active_tol is None and mpc.nx == 17 and mpc.cfg.boxed and mpc.cfg.dtype != 'f64':
            raise ValueError('feedback=True on an f32 17/6 input-box handle needs active_tol (solve_iterate_gains)')
        return _held_loop(mpc, x0, x_ref, u_ref, nsim, wind, plant_T, xbar, ubar, h, feedback, active_tol, wkw,
                          mkw, pkw, w17)
    if active_tol is not None:
        raise ValueError('active_tol belongs to feedback=True')
    dev = f'cuda:{mpc.device}'
    dt = mpc.dtype
    x = torch.as_tensor(x0, dtype=dt, device=dev).contiguous()
    B, N = x.shape[0], mpc.cfg.N
    NX, NU = mpc.nx, mpc.nu
    xb = torch.zeros((B, N + 1, NX), dtype=dt, device=dev) if xbar is None else \
        torch.as_tensor(xbar, dtype=dt, device=dev).clone()
    ub = torch.zeros((B, N, NU), dtype=dt, device=dev) if ubar is None else \
        torch.as_tensor(ubar, dtype=dt, device=dev).clone()
    u0 = torch.empty((B, NU), dtype=dt, device=dev)
    st = torch.empty((B,), dtype=torch.int32, device=dev)
    worst = torch.zeros((B,), dtype=torch.int32, device=dev)
    Xs = torch.empty((B, nsim + 1, NX), dtype=dt, device=dev)
    Us = torch.empty((B, nsim, NU), dtype=dt, device=dev)
    Xs[:, 0] = x
    stat = mpc.cfg.lbx is None
    diag = {k: torch.empty((B, nsim), dtype=dt, device=dev)
            for k in ('cost', 'res_eq') + (('res_stat',) if stat else ())} if diagnostics else None
    for i in range(nsim):
        if w17 is not None:
            mpc.solve_iterate_pw17(x, xb, ub, x_ref, u_ref, out=(u0, xb, ub, st), **w17)
        else:
            mpc.solve_iterate(x, xb, ub, x_ref, u_ref, wind=wind, out=(u0, xb, ub, st), **wkw, **mkw)
        worst = torch.maximum(worst, st)
        Us[:, i] = u0
        if diagnostics:
            ev = mpc.evaluate(xb, ub, x_ref, u_ref, x0=x, wind=wind, stat=stat)
            for k, v in diag.items():
                v[:, i] = ev[k]
        x = mpc.sim_step(x, u0, T=plant_T, wind=wind, **pkw)
        Xs[:, i + 1] = x
    if diagnostics:
        return Xs, Us, worst, diag
    return Xs, Us, worst


def _weights17_arg(mpc, weights17, wind):
    """The ``weights17`` dict of the loops, checked: None, or the keyword arguments of the pw17 entries."""
    if weights17 is None:
        return None
    if mpc.nx != 17:
        raise ValueError('weights17 covers the 17/6 model only (12/4: weights)')
    unknown = set(weights17) - {'Q', 'R', 'QN'}
    if unknown:
        raise ValueError(f'weights17: unknown keys {sorted(unknown)} (expected Q, R, QN)')
    if wind is not None:
        raise ValueError('wind is a 12/4-model extension')
    return {k: v for k, v in weights17.items() if v is not None}


def _held_loop(mpc, x0, x_ref, u_ref, nsim, wind, plant_T, xbar, ubar, h, feedback, active_tol, wkw, mkw, pkw,
               w17=None):
    """closed_loop with a solve every h plant steps and, optionally, the feedback law between."""
    import numpy as np
    import torch
    dev = f'cuda:{mpc.device}'
    dt = mpc.dtype
    x = torch.as_tensor(x0, dtype=dt, device=dev).contiguous()
    B, N = x.shape[0], mpc.cfg.N
    NX, NU = mpc.nx, mpc.nu
    xb = torch.zeros((B, N + 1, NX), dtype=dt, device=dev) if xbar is None else \
        torch.as_tensor(xbar, dtype=dt, device=dev).clone()
    ub = torch.zeros((B, N, NU), dtype=dt, device=dev) if ubar is None else \
        torch.as_tensor(ubar, dtype=dt, device=dev).clone()
    u0 = torch.empty((B, NU), dtype=dt, device=dev)
    st = torch.empty((B,), dtype=torch.int32, device=dev)
    worst = torch.zeros((B,), dtype=torch.int32, device=dev)
    Xs = torch.empty((B, nsim + 1, NX), dtype=dt, device=dev)
    Us = torch.empty((B, nsim, NU), dtype=dt, device=dev)
    Xs[:, 0] = x
    box = mpc.cfg.boxed
    if box:
        lb = torch.as_tensor(np.broadcast_to(np.asarray(mpc.cfg.lbu, dtype=np.float64), (NU,)).copy(),
                             dtype=dt, device=dev)
        hb = torch.as_tensor(np.broadcast_to(np.asarray(mpc.cfg.ubu, dtype=np.float64), (NU,)).copy(),
                             dtype=dt, device=dev)
    K = None
    for i in range(nsim):
        j = i % h
        if j == 0:
            if feedback:
                xb0, ub0 = xb.clone(), ub.clone()   # the solve overwrites the iterate in place
            if w17 is not None:
                mpc.solve_iterate_pw17(x, xb, ub, x_ref, u_ref, out=(u0, xb, ub, st), **w17)
            else:
                mpc.solve_iterate(x, xb, ub, x_ref, u_ref, wind=wind, out=(u0, xb, ub, st), **wkw, **mkw)
            worst = torch.maximum(worst, st)
            if feedback:
                g = mpc.solve_iterate_gains(xb0, ub0, U=ub if box else None, wind=wind, want_P0=False,
                                            active_tol=active_tol if box else None, **mkw)
                worst = torch.maximum(worst, g['status'])
                K = g['K']
        u = ub[:, j]
        if feedback:
            u = u + torch.einsum('bmi,bi->bm', K[:, j], x - xb[:, j])
        if box:
            u = torch.minimum(torch.maximum(u, lb), hb)
        u = u.contiguous()
        Us[:, i] = u
        x = mpc.sim_step(x, u, T=plant_T, wind=wind, **pkw)
        Xs[:, i + 1] = x
    return Xs, Us, worst


def closed_loop_diff(mpc: BatchedMPC, x0, x_ref, u_ref, nsim: int, xbar, ubar, wind=None, plant_T=None,
                     weights=None, plant_model=None, warm_start=True, plant_params=None, active_tol=None,
                     weights17=None, state_active_tol=None):
    """The loop of ``closed_loop`` as a differentiable torch operation: returns
    (X_sim [B, nsim+1, 12], U_sim [B, nsim, 4], status [B] = max over steps; 17 and 6 on the full
    model).  Each step is ``solve_iterate_diff`` followed by ``sim_step_diff`` (``sim_step_diff17`` on
    the 17/6 model; ``mpc_blaster_amd.autograd``), so a loss on
    X_sim, U_sim can be differentiated with respect to the torch tensors ``x0``, ``x_ref``, ``u_ref``,
    the tensors in ``weights`` and ``plant_model``.  The forward values are ``closed_loop``'s with
    the same arguments: the same entry points in the same order.

    ``weights``: a dict with any of the keys ``Q``, ``R``, ``QN`` as in ``closed_loop``.  They always go
    to the solve as per-instance arguments (``per_instance_weights=True``), so a ``[1, n]`` row receives
    the sum over the batch; installing them on the handle cannot be chained over several steps.
    ``plant_model``: vehicle records [B|1, 14] of the plant (``sim_step_diff``'s rule for the gradient).
    ``wind``, ``xbar``, ``ubar`` and the controller's own vehicle are constants; there is no ``model=``
    argument, because the RTI step's gradients have no per-instance model.

    ``warm_start=True``: the next step linearises at the detached (X, U) of this one, the persistent
    iterate of ``closed_loop``.  That is the RTI / Gauss-Newton convention: the gradient ignores the
    path through the iterate.  ``warm_start=False``: every step linearises at the given
    (``xbar``, ``ubar``); the loop is then piecewise smooth in the differentiated inputs and the
    gradient is exact on the active sets of the forward pass.  An instance whose solve reports a
    status other than 0 at some step passes no gradient through that solve.

    The 17/6 model.  The loop chains ``solve_iterate_diff`` with ``sim_step_diff17`` and is
    differentiable in ``x0``, ``x_ref``, ``u_ref`` and ``plant_params`` (the plant's parameter vectors
    [25] or [B|1, 25], ``closed_loop``'s argument; a one-row tensor receives the batch sum).
    ``active_tol`` is ``solve_iterate_diff``'s active-set tolerance.  The controller's parameters are
    the handle's ``set_params`` and constants.  ``weights17``: a dict with any of ``Q``, ``R``, ``QN`` as
    in ``closed_loop``; every solve is then ``solve_iterate_diff_pw17``, whose weights are arguments of
    the solve and of its backward pass, so the loop is differentiable in the per-instance Q, R, QN as
    well (a ``[1, ...]`` tensor receives the batch sum), and several forward graphs on one handle can
    each be differentiated.  Refused with ``ValueError``: ``weights`` (the 12/4 keyword: without
    per-instance arguments the weights are installed on the handle, so every forward pass would
    invalidate the previous step's backward), ``plant_model``, ``wind``, and a handle with the state
    box unless ``state_active_tol`` is given: that is ``solve_iterate_diff``'s tolerance of the active
    state rows, passed to every solve of the loop, whose backward pass is then the product with
    state rows (``mpcb_solve_vjp17_sx``).  On a 12/4 handle ``plant_params``, ``active_tol``,
    ``weights17`` and ``state_active_tol`` are refused."""
    import torch
    from .autograd import sim_step_diff, sim_step_diff17, solve_iterate_diff, solve_iterate_diff_pw17
    full = mpc.nx == 17
    if full:
        if weights is not None:
            raise ValueError('closed_loop_diff on the 17/6 model takes no weights: they are installed on the '
                             'handle, and every forward pass would invalidate the previous step\'s backward')
        if plant_model is not None:
            raise ValueError('plant_model covers the 12/4 model only (17/6: plant_params)')
        if wind is not None:
            raise ValueError('wind is a 12/4-model extension')
        if mpc.cfg.lbx is not None and state_active_tol is None:
            raise ValueError('closed_loop_diff does not cover the 17/6 state box (solve_iterate_diff)')
    elif plant_params is not None or active_tol is not None or state_active_tol is not None:
        raise ValueError('plant_params and active_tol belong to the 17/6 model')
    w17 = _weights17_arg(mpc, weights17, wind)
    wkw = {}
    if weights is not None:
        unknown = set(weights) - {'Q', 'R', 'QN'}
        if unknown:
            raise ValueError(f'weights: unknown keys {sorted(unknown)} (expected Q, R, QN)')
        wkw = {k: v for k, v in weights.items() if v is not None}
    dev, dt = f'cuda:{mpc.device}', mpc.dtype
    x = torch.as_tensor(x0, dtype=dt, device=dev).contiguous()
    xb = torch.as_tensor(xbar, dtype=dt, device=dev).detach().clone()
    ub = torch.as_tensor(ubar, dtype=dt, device=dev).detach().clone()
    worst = torch.zeros((x.shape[0],), dtype=torch.int32, device=dev)
    Xs, Us = [x], []
    skw = {} if state_active_tol is None else dict(state_active_tol=state_active_tol)
    for _ in range(nsim):
        if w17 is not None:
            u0, X, U = solve_iterate_diff_pw17(mpc, x, xb, ub, x_ref, u_ref, active_tol=active_tol, **w17, **skw)
        elif full:
            u0, X, U = solve_iterate_diff(mpc, x, xb, ub, x_ref, u_ref, active_tol=active_tol, **skw)
        else:
            u0, X, U = solve_iterate_diff(mpc, x, xb, ub, x_ref, u_ref, wind=wind, per_instance_weights=bool(wkw),
                                          **wkw)
        worst = torch.maximum(worst, mpc.get_status())
        if warm_start:
            xb, ub = X.detach(), U.detach()
        if full:
            x = sim_step_diff17(mpc, x, u0, T=plant_T, params=plant_params)
        else:
            x = sim_step_diff(mpc, x, u0, T=plant_T, wind=wind, model=plant_model)
        Xs.append(x)
        Us.append(u0)
    return torch.stack(Xs, dim=1), torch.stack(Us, dim=1), worst
