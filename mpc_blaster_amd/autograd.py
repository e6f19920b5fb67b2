"""The SQP_RTI step as a differentiable torch operation.

``solve_iterate_diff(mpc, x0, xbar, ubar, x_ref, u_ref, wind=None, Q=None, R=None, QN=None,
active_tol=None) -> (u0, X, U)`` runs ``BatchedMPC.solve_iterate`` in the forward pass and one
``mpcb_solve_vjp`` call (``mpcb_solve_vjp17`` on the 17/6 model;
``mpcb_solve_vjp_w`` when a weight gradient is needed; include/mpcb.h) in the backward pass,
so a loss on ``u0``, ``X``, ``U`` can be differentiated with respect to ``x0``, ``x_ref``, ``u_ref``
and the cost weights.

What the gradient is.  In iterate mode the linearisation point (xbar, ubar) does not depend on the
differentiated inputs, so (X, U) is affine in them, piecewise affine with the input box, and the
gradient is exact on the active set of the forward solve (at a degenerate point, a clamped
component with a zero multiplier, it is one of the valid one-sided derivatives).  The active set
is read from U (a component on a bound is clamped): an instance the solver handed to its interior
point has U strictly inside the box and gets the unconstrained gradient (include/mpcb.h).  ``xbar``,
``ubar`` and ``wind`` are constants (Gauss-Newton / RTI): their gradients are ``None``, as is that
of the model.  An instance whose forward status is not 0 gets zero gradients.  A
reference passed as one row (``[1, ...]`` or without a batch axis) receives the sum of the
per-instance gradients.  Not differentiable twice.

The 17/6 model (``mpcb_solve_vjp17``).  Its boxes are solved by an interior point, so U lies near
its bounds and the active set is taken by tolerance: the forward pass derives the mask
``(U <= lbu + active_tol) | (U >= ubu - active_tol)`` once (``BatchedMPC.active_mask17``: 1e-6 on an
f64 handle, required on an f32 one) and the backward pass hands it to the kernel, which is exact
for that mask.  ``wind`` raises as in ``solve_iterate``.  The weights work as on 12/4.

The 17/6 state box (``mpcb_solve_vjp17_sx``).  An active state row is a state equality of the adjoint
problem, so a handle with ``lbx`` / ``ubx`` is refused unless ``state_active_tol`` is given (f64 only,
as the state box itself).  Then the forward pass derives both masks once, the inputs' from U and the
state rows' from X (``BatchedMPC.active_mask17x``: ``X <= lbx + tol`` or ``X >= ubx - tol`` on stages
1..N-1; the polished rows sit within 1e-10 of their bounds, 1e-6 is the reference's tolerance), and
the backward pass is the product with those rows held at zero: exact on that active set.  An
instance gets zero gradients when its forward status is not 0, as everywhere, and also when the
product's own status is not 0: MPCB_STATUS_MAXITER there marks a (nearly) dependent active set, at
which the solve is not differentiable.  Without ``state_active_tol`` every call behaves as before.

The weights.  ``Q``, ``R``, ``QN`` are optional torch tensors: a vector (the diagonal) or a
symmetric matrix.  The weights belong to the handle, so the forward pass installs the value of
every weight tensor it is given with ``mpc.set_weights`` before it solves: that reads the tensor
on the host (a synchronisation) and waits for the device, and the handle keeps the new weights
afterwards.  The backward pass returns, for each weight tensor, the gradient summed over the
instances with forward status 0, in the tensor's shape and dtype: the symmetric matrix gQ of
include/mpcb.h for a matrix (so that dL = <gQ, dQ> for a symmetric dQ), its diagonal for a vector.
It is exact on the active set at fixed (xbar, ubar), like the others.

Handle state between forward and backward.  Every gradient of the step, ``x0``'s, ``x_ref``'s and
``u_ref``'s as much as the weights', is taken at the handle's Q, R, QN and vehicle, which the
backward pass reads from the handle when it runs.  Every forward pass therefore records the
handle's weights version and its model version (``BatchedMPC._weights_version``, bumped by
``set_weights``, hence also by another forward pass with weight tensors; ``_model_version``, bumped
by ``set_t_blast`` and ``set_params``), with or without weight arguments, and the backward pass
raises ``RuntimeError`` naming the setter if either has moved: it never returns the gradient of a
problem the forward pass did not solve.  A comparison is left out exactly where the backward pass
does not read that state: the weights version with per-instance weights when all three of ``Q``,
``R``, ``QN`` are given (an omitted one falls back to the handle's), the model version in the plant
step with a ``model`` record.  Restore nothing by hand: run the forward pass again.

Weights per instance (``per_instance_weights=True``, 12/4 model).  ``Q``, ``R``, ``QN`` then carry a
batch axis: a 2-D tensor ``[B|1, n]`` holds diagonals, a 3-D tensor ``[B|1, n, n]`` symmetric
matrices (``BatchedMPC.solve_iterate``'s rule).  They are arguments of the solve
(``mpcb_solve_iterate_pw``) and of the backward pass (``mpcb_solve_vjp_pw``): the forward pass calls
neither ``set_weights`` nor anything that synchronises, and the handle's weights stay as they were.
Each weight tensor receives its gradient per instance in its own shape, the diagonal of gQ for a
2-D tensor, summed over the batch only for a ``[1, ...]`` tensor; instances with forward status
other than 0 get zeros.  With the input box the solve is the plain active set of
``mpcb_solve_iterate_pw`` (fp64 only).  A 17/6 handle raises ``ValueError``.

Weights per instance on the 17/6 model.  ``solve_iterate_diff_pw17(mpc, x0, xbar, ubar, x_ref, u_ref,
Q=None, R=None, QN=None, active_tol=None) -> (u0, X, U)`` runs ``BatchedMPC.solve_iterate_pw17`` in the
forward pass and one ``solve_iterate_vjp_pw17`` call (``mpcb_solve_vjp_pw17``) in the backward pass,
with the conventions of the paragraph above: the weight tensors follow the batch-axis rule, each
receives its gradient in its own shape (the diagonal of gQ for a 2-D tensor, the batch sum for a
``[1, ...]`` tensor), instances with forward status other than 0 get zeros, the handle's weights are
neither read (when all three are given) nor changed, so two forward graphs on one handle can both
be differentiated.  The weights-version check is left out exactly when all three are given; the
model-version check stays (``set_params``).  The mask is derived once by ``active_tol`` as for
``solve_iterate_diff`` on 17/6; the state-box handle without ``state_active_tol`` (with it: the
paragraph on the state box above, word for word) and the f32 boxed handle without ``active_tol``
are refused as there.  A 12/4 handle raises ``ValueError``.

The plant step.  ``sim_step_diff(mpc, x, u, T=None, wind=None, model=None) -> x_out`` runs
``BatchedMPC.sim_step`` in the forward pass and one ``mpcb_sim_step_vjp`` call in the backward pass,
which requests exactly the outputs whose inputs need a gradient: ``x``, ``u``, ``wind`` and ``model``
(the vehicle records of ``pack_model``).  It is the exact derivative of the discrete RK4 step.  A
``[1, 3]`` (or ``[3]``) wind and a ``[1, 14]`` (or ``[14]``) model receive the sum over the batch, in
the tensor's shape and dtype; rows wider than 14 get zeros in the pad columns.  The model gradient
follows include/mpcb.h: entry 0 is d/d mass, the nine entries of J are independent.  ``T`` and
gravity carry no gradient.  Without ``model`` the step is the handle's vehicle's, so ``set_t_blast``
between forward and backward raises ``RuntimeError`` (above); with a record it goes through.  12/4
model only (a 17/6 handle raises ``ValueError``); not differentiable
twice.

The 17/6 plant step.  ``sim_step_diff17(mpc, x, u, T=None, params=None) -> x_out`` runs
``BatchedMPC.sim_step(params=)`` in the forward pass and one ``mpcb_sim_step_vjp17`` call in the
backward pass, which requests exactly the outputs whose inputs need a gradient: ``x``, ``u`` and
``params`` (the plant's 25-vectors in the layout of ``set_params``; entry 24 is T_blast).  A
``[25]`` or ``[1, 25]`` tensor receives the sum over the batch, in its own shape and dtype; rows wider
than 25 get zeros in the pad columns.  Mass, J, the arms, gravity and ``T`` carry no gradient: they
are the handle's.  Without ``params`` the step reads the handle's ``set_params`` rows, so
``set_params`` or ``set_t_blast`` between forward and backward raises ``RuntimeError`` (above); with a
``params`` tensor it goes through.  A 12/4 handle raises ``ValueError``.

torch is imported on first use, as in ``api.py``.
"""
from __future__ import annotations

_FN = None


def _same_weights(mpc, version):
    if mpc._weights_version != version:
        raise RuntimeError('the weights of the MPC handle changed after the forward pass (set_weights, or '
                           'another forward pass with weight tensors): every gradient of the step needs the '
                           'weights the forward pass solved with')


def _same_model(mpc, version):
    if mpc._model_version != version:
        raise RuntimeError(f'{mpc._model_setter} changed the vehicle of the MPC handle after the forward pass: '
                           'the gradient needs the model the forward pass ran with')


def _function():
    global _FN
    if _FN is not None:
        return _FN
    import torch
    from torch.autograd.function import once_differentiable

    class SolveIterate(torch.autograd.Function):
        @staticmethod
        def forward(ctx, mpc, x0, xbar, ubar, x_ref, u_ref, wind, Q, R, QN, active_tol, pw, state_active_tol):
            N = mpc.cfg.N
            full = mpc.nx == 17
            if pw and full:
                raise ValueError('per_instance_weights covers the 12/4 model only')
            if full and mpc.cfg.lbx is not None and state_active_tol is None:
                raise ValueError('solve_iterate_diff does not cover the 17/6 state box: an active state row '
                                 'is a state equality of the adjoint problem (use a handle without lbx/ubx '
                                 'when no state row is active)')
            if full and mpc.cfg.boxed and active_tol is None and mpc.cfg.dtype != 'f64':
                raise ValueError('active_tol is required on an f32 17/6 input-box handle')
            x0d, _ = mpc._dev(x0.detach(), (mpc.nx,), 'x0')
            B = x0d.shape[0]
            xb, _ = mpc._dev(xbar.detach() if torch.is_tensor(xbar) else xbar, (N + 1, mpc.nx), 'xbar', B)
            ub, _ = mpc._dev(ubar.detach() if torch.is_tensor(ubar) else ubar, (N, mpc.nu), 'ubar', B)
            wd = None
            if wind is not None:
                wd, _ = mpc._dev(wind.detach() if torch.is_tensor(wind) else wind, (3,), 'wind', B,
                                 allow_broadcast=True)
            wts = (Q, R, QN)
            ctx.has_weights = any(w is not None for w in wts)
            ctx.pw = bool(pw) and ctx.has_weights
            wdet = [None if w is None else w.detach() for w in wts]
            if ctx.pw:   # arguments of the solve: the handle keeps its weights
                u0 = mpc.solve_iterate(x0d, xb, ub, x_ref.detach(), u_ref.detach(), wind=wd, Q=wdet[0], R=wdet[1],
                                       QN=wdet[2])
            else:
                if ctx.has_weights:
                    mpc.set_weights(*wts)
                u0 = mpc.solve_iterate(x0d, xb, ub, x_ref.detach(), u_ref.detach(), wind=wd)   # fresh outputs
            X, U, status = mpc.get_state_trajectory(), mpc.get_input_trajectory(), mpc.get_status()
            ctx.mpc = mpc
            ctx.full = full
            # (17/6) the active set by tolerance, derived once from the forward solve's U
            ctx.fixed = mpc.active_mask17(U, active_tol) if full else None
            # ... and, with the state box, the active state rows from its X
            ctx.fixed_x = mpc.active_mask17x(X, state_active_tol) if full and state_active_tol is not None else None
            ctx.shapes = (tuple(x0.shape), tuple(x_ref.shape), tuple(u_ref.shape))
            ctx.dtypes = (x0.dtype, x_ref.dtype, u_ref.dtype)
            ctx.has_wind = wd is not None
            saved = [xb, ub, U, status] + ([wd] if wd is not None else [])
            # the handle state the backward pass will read again (module docstring)
            ctx.wversion, ctx.mversion = mpc._weights_version, mpc._model_version
            if ctx.has_weights:
                ctx.wmeta = [None if w is None else (tuple(w.shape), w.dtype) for w in wts]
                saved += [X, x_ref.detach(), u_ref.detach()]
            if ctx.pw:
                ctx.wpresent = [w is not None for w in wdet]
                saved += [w for w in wdet if w is not None]
            ctx.save_for_backward(*saved)
            return u0, X, U

        @staticmethod
        @once_differentiable
        def backward(ctx, g_u0, g_X, g_U):
            mpc = ctx.mpc
            xb, ub, U, status = ctx.saved_tensors[:4]
            wd = ctx.saved_tensors[4] if ctx.has_wind else None
            need = ctx.needs_input_grad
            kw = dict(fixed=ctx.fixed) if ctx.full else dict(wind=wd)
            if ctx.fixed_x is not None:
                kw['fixed_x'] = ctx.fixed_x
            want_w = ctx.has_weights and any(need[7:10])
            if not (ctx.pw and all(ctx.wpresent)):
                _same_weights(mpc, ctx.wversion)
            _same_model(mpc, ctx.mversion)
            gU = g_U.to(mpc.dtype).clone()
            gU[:, 0] += g_u0.to(mpc.dtype)
            pwkw = {}
            nsaved = len(ctx.saved_tensors)
            if ctx.pw:
                given = iter(ctx.saved_tensors[nsaved - sum(ctx.wpresent):])
                pwkw = {k: next(given) for k, p in zip(('Q', 'R', 'QN'), ctx.wpresent) if p}
                nsaved -= sum(ctx.wpresent)
            if ctx.pw and want_w:
                X, xr, ur = ctx.saved_tensors[nsaved - 3:nsaved]
                out = mpc.solve_iterate_vjp(xb, ub, gX=g_X, gU=gU, U=U, X=X, x_ref=xr, u_ref=ur, weights=True,
                                            wind=wd, **pwkw)
            elif ctx.pw:
                out = mpc.solve_iterate_vjp(xb, ub, gX=g_X, gU=gU, U=U, wind=wd, **pwkw)
            elif want_w:
                X, xr, ur = ctx.saved_tensors[-3:]
                out = mpc.solve_iterate_vjp(xb, ub, gX=g_X, gU=gU, U=U, X=X, x_ref=xr, u_ref=ur, weights=True,
                                            **kw)
            else:
                out = mpc.solve_iterate_vjp(xb, ub, gX=g_X, gU=gU, U=None if ctx.full else U, **kw)
            ok = status == 0
            if ctx.fixed_x is not None:   # (a product that did not converge: module docstring)
                ok = ok & (out['status'] == 0)
            grads = []
            for g, shape, dt in zip((out['gx0'], out['gxref'], out['guref']), ctx.shapes, ctx.dtypes):
                g = torch.where(ok.reshape(-1, *([1] * (g.dim() - 1))), g, torch.zeros_like(g))
                if len(shape) < g.dim() or shape[0] != g.shape[0]:
                    g = g.sum(dim=0, keepdim=True)   # one row for the whole batch
                grads.append(g.reshape(shape).to(dt))
            wgrads = [None, None, None]
            if want_w:
                for i, key in enumerate(('gQ', 'gR', 'gQN')):
                    if ctx.wmeta[i] is None or not need[7 + i]:
                        continue
                    shape, dt = ctx.wmeta[i]
                    g = torch.where(ok.reshape(-1, 1, 1), out[key], torch.zeros_like(out[key]))
                    if ctx.pw:   # per instance, in the tensor's shape; one row: the batch sum
                        g = torch.diagonal(g, dim1=1, dim2=2) if len(shape) == 2 else g
                        if shape[0] == 1 and g.shape[0] != 1:
                            g = g.sum(dim=0, keepdim=True)
                        wgrads[i] = g.reshape(shape).to(dt)
                        continue
                    g = g.sum(dim=0)
                    wgrads[i] = (torch.diagonal(g) if len(shape) == 1 else g).reshape(shape).to(dt)
            return (None, grads[0] if need[1] else None, None, None, grads[1] if need[4] else None,
                    grads[2] if need[5] else None, None, *wgrads, None, None, None)

    _FN = SolveIterate
    return _FN


_PW17 = None


def _pw17_function():
    global _PW17
    if _PW17 is not None:
        return _PW17
    import numpy as np
    import torch
    from torch.autograd.function import once_differentiable

    class SolveIteratePw17(torch.autograd.Function):
        @staticmethod
        def forward(ctx, mpc, x0, xbar, ubar, x_ref, u_ref, Q, R, QN, active_tol, state_active_tol):
            N = mpc.cfg.N
            if mpc.nx != 17:
                raise ValueError('solve_iterate_diff_pw17 covers the 17/6 model only (12/4: solve_iterate_diff with '
                                 'per_instance_weights=True)')
            if mpc.cfg.lbx is not None and state_active_tol is None:
                raise ValueError('solve_iterate_diff_pw17 does not cover the 17/6 state box: an active state row '
                                 'is a state equality of the adjoint problem (use a handle without lbx/ubx '
                                 'when no state row is active)')
            if mpc.cfg.boxed and active_tol is None and mpc.cfg.dtype != 'f64':
                raise ValueError('active_tol is required on an f32 17/6 input-box handle')
            x0d, _ = mpc._dev(x0.detach(), (mpc.nx,), 'x0')
            B = x0d.shape[0]
            xb, _ = mpc._dev(xbar.detach() if torch.is_tensor(xbar) else xbar, (N + 1, mpc.nx), 'xbar', B)
            ub, _ = mpc._dev(ubar.detach() if torch.is_tensor(ubar) else ubar, (N, mpc.nu), 'ubar', B)
            wts = (Q, R, QN)
            # (a weight that is no tensor is a constant: an array, on the device once)
            wdet = [None if w is None else w.detach() if torch.is_tensor(w) else
                    torch.tensor(np.asarray(w), dtype=mpc.dtype, device=mpc._tdev) for w in wts]
            u0 = mpc.solve_iterate_pw17(x0d, xb, ub, x_ref.detach(), u_ref.detach(), Q=wdet[0], R=wdet[1],
                                        QN=wdet[2])   # fresh outputs; the handle keeps its weights
            X, U, status = mpc.get_state_trajectory(), mpc.get_input_trajectory(), mpc.get_status()
            ctx.mpc = mpc
            ctx.fixed = mpc.active_mask17(U, active_tol)   # by tolerance, once, from the forward solve's U
            ctx.fixed_x = None if state_active_tol is None else mpc.active_mask17x(X, state_active_tol)
            ctx.shapes = (tuple(x0.shape), tuple(x_ref.shape), tuple(u_ref.shape))
            ctx.dtypes = (x0.dtype, x_ref.dtype, u_ref.dtype)
            ctx.wversion, ctx.mversion = mpc._weights_version, mpc._model_version
            ctx.wmeta = [(tuple(w.shape), w.dtype) if torch.is_tensor(w) else None for w in wts]
            ctx.wpresent = [w is not None for w in wdet]
            ctx.save_for_backward(xb, ub, U, status, X, x_ref.detach(), u_ref.detach(),
                                  *(w for w in wdet if w is not None))
            return u0, X, U

        @staticmethod
        @once_differentiable
        def backward(ctx, g_u0, g_X, g_U):
            mpc = ctx.mpc
            xb, ub, U, status, X, xr, ur = ctx.saved_tensors[:7]
            given = iter(ctx.saved_tensors[7:])
            pwkw = {k: next(given) for k, p in zip(('Q', 'R', 'QN'), ctx.wpresent) if p}
            need = ctx.needs_input_grad
            want_w = any(need[6:9])
            if not all(ctx.wpresent):   # an omitted matrix is the handle's
                _same_weights(mpc, ctx.wversion)
            _same_model(mpc, ctx.mversion)
            gU = g_U.to(mpc.dtype).clone()
            gU[:, 0] += g_u0.to(mpc.dtype)
            if ctx.fixed_x is not None:
                pwkw['fixed_x'] = ctx.fixed_x
            if want_w:
                out = mpc.solve_iterate_vjp_pw17(xb, ub, gX=g_X, gU=gU, U=U, X=X, x_ref=xr, u_ref=ur, weights=True,
                                                 fixed=ctx.fixed, **pwkw)
            else:
                out = mpc.solve_iterate_vjp_pw17(xb, ub, gX=g_X, gU=gU, fixed=ctx.fixed, **pwkw)
            ok = status == 0
            if ctx.fixed_x is not None:   # (a product that did not converge: module docstring)
                ok = ok & (out['status'] == 0)
            grads = []
            for g, shape, dt in zip((out['gx0'], out['gxref'], out['guref']), ctx.shapes, ctx.dtypes):
                g = torch.where(ok.reshape(-1, *([1] * (g.dim() - 1))), g, torch.zeros_like(g))
                if len(shape) < g.dim() or shape[0] != g.shape[0]:
                    g = g.sum(dim=0, keepdim=True)   # one row for the whole batch
                grads.append(g.reshape(shape).to(dt))
            wgrads = [None, None, None]
            if want_w:
                for i, key in enumerate(('gQ', 'gR', 'gQN')):
                    if ctx.wmeta[i] is None or not need[6 + i]:
                        continue
                    shape, dt = ctx.wmeta[i]
                    g = torch.where(ok.reshape(-1, 1, 1), out[key], torch.zeros_like(out[key]))
                    g = torch.diagonal(g, dim1=1, dim2=2) if len(shape) == 2 else g
                    if shape[0] == 1 and g.shape[0] != 1:
                        g = g.sum(dim=0, keepdim=True)   # one row: the batch sum
                    wgrads[i] = g.reshape(shape).to(dt)
            return (None, grads[0] if need[1] else None, None, None, grads[1] if need[4] else None,
                    grads[2] if need[5] else None, *wgrads, None, None)

    _PW17 = SolveIteratePw17
    return _PW17


_SIM = None


def _sim_function():
    global _SIM
    if _SIM is not None:
        return _SIM
    import torch
    from torch.autograd.function import once_differentiable

    class SimStep(torch.autograd.Function):
        @staticmethod
        def forward(ctx, mpc, x, u, T, wind, model):
            if mpc.nx == 17:
                raise ValueError('sim_step_diff covers the 12/4 model only')
            xs, _ = mpc._dev(x.detach(), (mpc.nx,), 'x')
            B = xs.shape[0]
            us, _ = mpc._dev(u.detach(), (mpc.nu,), 'u', B)
            wd = md = None
            if wind is not None:
                wd, _ = mpc._dev(wind.detach() if torch.is_tensor(wind) else wind, (3,), 'wind', B,
                                 allow_broadcast=True)
            if model is not None:
                md, _ = mpc._model_arg(model.detach() if torch.is_tensor(model) else model, B)
            xo = mpc.sim_step(xs, us, T=T, wind=wd, model=md)
            ctx.mpc, ctx.T = mpc, T
            ctx.mversion = mpc._model_version   # read again by the backward pass unless a record is given
            ctx.has = (wd is not None, md is not None)
            ctx.meta = [(tuple(t.shape), t.dtype) if torch.is_tensor(t) else None for t in (x, u, wind, model)]
            ctx.save_for_backward(xs, us, *(t for t in (wd, md) if t is not None))
            return xo

        @staticmethod
        @once_differentiable
        def backward(ctx, g):
            mpc = ctx.mpc
            xs, us = ctx.saved_tensors[:2]
            rest = list(ctx.saved_tensors[2:])
            wd = rest.pop(0) if ctx.has[0] else None
            md = rest.pop(0) if ctx.has[1] else None
            need = [ctx.needs_input_grad[i] for i in (1, 2, 4, 5)]
            keys = ('gx', 'gu', 'gwind', 'gmodel')
            want = tuple(k for k, n in zip(keys, need) if n)
            grads = [None] * 4
            if want:
                if md is None:
                    _same_model(mpc, ctx.mversion)
                out = mpc.sim_step_vjp(xs, us, g.to(mpc.dtype), T=ctx.T, wind=wd, model=md, want=want)
                for i, k in enumerate(keys):
                    if k not in out:
                        continue
                    shape, dt = ctx.meta[i]
                    v = out[k]
                    rows = 1 if len(shape) == 1 else shape[0]
                    if rows == 1 and v.shape[0] != 1:
                        v = v.sum(dim=0, keepdim=True)   # one row for the whole batch
                    if k == 'gmodel' and shape[-1] > v.shape[1]:
                        v = torch.nn.functional.pad(v, (0, shape[-1] - v.shape[1]))   # pad columns: zeros
                    grads[i] = v.reshape(shape).to(dt)
            return (None, grads[0], grads[1], None, grads[2], grads[3])

    _SIM = SimStep
    return _SIM


_SIM17 = None


def _sim17_function():
    global _SIM17
    if _SIM17 is not None:
        return _SIM17
    import torch
    from torch.autograd.function import once_differentiable

    class SimStep17(torch.autograd.Function):
        @staticmethod
        def forward(ctx, mpc, x, u, T, params):
            if mpc.nx != 17:
                raise ValueError('sim_step_diff17 covers the 17/6 model only (12/4: sim_step_diff)')
            xs, _ = mpc._dev(x.detach(), (mpc.nx,), 'x')
            B = xs.shape[0]
            us, _ = mpc._dev(u.detach(), (mpc.nu,), 'u', B)
            pd = None
            if params is not None:
                pd, _ = mpc._params_arg(params.detach() if torch.is_tensor(params) else params, B)
            xo = mpc.sim_step(xs, us, T=T, params=pd)
            ctx.mpc, ctx.T = mpc, T
            ctx.mversion = mpc._model_version   # read again by the backward pass unless params is given
            ctx.has = pd is not None
            ctx.meta = [(tuple(t.shape), t.dtype) if torch.is_tensor(t) else None for t in (x, u, params)]
            ctx.save_for_backward(xs, us, *((pd,) if pd is not None else ()))
            return xo

        @staticmethod
        @once_differentiable
        def backward(ctx, g):
            mpc = ctx.mpc
            xs, us = ctx.saved_tensors[:2]
            pd = ctx.saved_tensors[2] if ctx.has else None
            need = [ctx.needs_input_grad[i] for i in (1, 2, 4)]
            keys = ('gx', 'gu', 'gparams')
            want = tuple(k for k, n in zip(keys, need) if n)
            grads = [None] * 3
            if want:
                if pd is None:
                    _same_model(mpc, ctx.mversion)
                out = mpc.sim_step_vjp17(xs, us, g.to(mpc.dtype), T=ctx.T, params=pd, want=want)
                for i, k in enumerate(keys):
                    if k not in out:
                        continue
                    shape, dt = ctx.meta[i]
                    v = out[k]
                    rows = 1 if len(shape) == 1 else shape[0]
                    if rows == 1 and v.shape[0] != 1:
                        v = v.sum(dim=0, keepdim=True)   # one row for the whole batch
                    if k == 'gparams' and shape[-1] > v.shape[1]:
                        v = torch.nn.functional.pad(v, (0, shape[-1] - v.shape[1]))   # pad columns: zeros
                    grads[i] = v.reshape(shape).to(dt)
            return (None, grads[0], grads[1], None, grads[2])

    _SIM17 = SimStep17
    return _SIM17


def sim_step_diff17(mpc, x, u, T=None, params=None):
    """x_out [B,17] of ``mpc.sim_step(params=)`` on the 17/6 model, differentiable with respect to the
    torch tensors ``x``, ``u`` and ``params`` (module docstring)."""
    import torch
    x, u = (t if torch.is_tensor(t) else torch.as_tensor(t, dtype=mpc.dtype, device=mpc._tdev) for t in (x, u))
    return _sim17_function().apply(mpc, x, u, T, params)


def sim_step_diff(mpc, x, u, T=None, wind=None, model=None):
    """x_out [B,12] of ``mpc.sim_step``, differentiable with respect to the torch tensors ``x``, ``u``,
    ``wind`` and ``model`` (module docstring)."""
    import torch
    x, u = (t if torch.is_tensor(t) else torch.as_tensor(t, dtype=mpc.dtype, device=mpc._tdev) for t in (x, u))
    return _sim_function().apply(mpc, x, u, T, wind, model)


def solve_iterate_diff(mpc, x0, xbar, ubar, x_ref, u_ref, wind=None, Q=None, R=None, QN=None,
                       active_tol=None, per_instance_weights=False, state_active_tol=None):
    """(u0 [B,4], X [B,N+1,12], U [B,N,4]; 17 and 6 on the full model) of ``mpc.solve_iterate``,
    differentiable with respect to the torch tensors ``x0``, ``x_ref`` and ``u_ref`` and, when given, the weight tensors ``Q``, ``R``,
    ``QN`` (vectors or symmetric matrices; installed on the handle by the forward pass, a host
    synchronisation: module docstring).  ``active_tol``: the 17/6 active-set tolerance (module
    docstring).  ``per_instance_weights=True``: the weight tensors carry a batch axis and are arguments
    of the solve, not installed on the handle (module docstring).  ``state_active_tol``: the tolerance of
    the active state rows on a 17/6 state-box handle, which is refused without it; an instance whose
    product does not converge (status not 0) gets zero gradients (module docstring).  The per-instance
    status is ``mpc.get_status()``."""
    import torch
    x0, x_ref, u_ref = (t if torch.is_tensor(t) else torch.as_tensor(t, dtype=mpc.dtype, device=mpc._tdev)
                        for t in (x0, x_ref, u_ref))
    return _function().apply(mpc, x0, xbar, ubar, x_ref, u_ref, wind, Q, R, QN, active_tol,
                             bool(per_instance_weights), state_active_tol)


def solve_iterate_diff_pw17(mpc, x0, xbar, ubar, x_ref, u_ref, Q=None, R=None, QN=None, active_tol=None,
                            state_active_tol=None):
    """(u0 [B,6], X [B,N+1,17], U [B,N,6]) of ``mpc.solve_iterate_pw17``, differentiable with respect to
    the torch tensors ``x0``, ``x_ref``, ``u_ref`` and the per-instance weight tensors ``Q``, ``R``, ``QN``
    (2-D diagonals or 3-D matrices with a batch axis; arguments of the solve, not installed on the
    handle: module docstring).  ``active_tol``: the 17/6 active-set tolerance.  ``state_active_tol``: the
    tolerance of the active state rows on a state-box handle, which is refused without it; an instance
    whose product does not converge (status not 0) gets zero gradients.  The per-instance status is
    ``mpc.get_status()``."""
    import torch
    x0, x_ref, u_ref = (t if torch.is_tensor(t) else torch.as_tensor(t, dtype=mpc.dtype, device=mpc._tdev)
                        for t in (x0, x_ref, u_ref))
    return _pw17_function().apply(mpc, x0, xbar, ubar, x_ref, u_ref, Q, R, QN, active_tol, state_active_tol)
