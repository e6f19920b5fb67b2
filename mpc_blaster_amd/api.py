"""Batch API over the HIP library: ``solve(x0, x_ref, u_ref)`` / ``get_control()``.

This is the north_star call surface for the per-control-step solve that the reference runs
one instance at a time through ``ocp_solver.solve()`` (src/scripts/simulation_blaster.py:80).
Device buffers are torch ROCm tensors (plumbing only); every computation runs in
libmpcblaster.so.  Calls are asynchronous on torch's current stream; results are valid once
that stream is synchronised (``torch.cuda.synchronize()`` or reading them on the host).
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib
from .config import MPCConfig


def _torch():
    import torch
    return torch


class BatchedMPC:
    """A handle bound to one GPU holding the workspace for up to ``max_batch`` instances."""

    def __init__(self, config: MPCConfig, max_batch: int, device: int | None = None):
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError('BatchedMPC needs a ROCm GPU (torch.cuda.is_available() is False)')
        self.lib = _lib.load()
        self.cfg = config
        self.device = torch.cuda.current_device() if device is None else int(device)
        self._tdev = torch.device('cuda', self.device)
        self.max_batch = int(max_batch)
        self._c = config.to_c()
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mpcb_create(ctypes.byref(self._c), self.device, self.max_batch,
                                            ctypes.byref(h)))
        self._h = h
        self.dtype = config.torch_dtype
        self.nx, self.nu = config.nx, config.nu
        self._u0 = self._X = self._U = self._status = None
        self._params = None
        self._weights_version = 0   # bumped by set_weights (autograd checks it in backward)
        self._model_version = 0     # bumped by set_t_blast and set_params (likewise)
        self._model_setter = None   # ... and the name of the one that moved it last

    # ------------------------------------------------------------------ helpers
    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self.lib.mpcb_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def workspace_bytes(self) -> int:
        return int(self.lib.mpcb_workspace_bytes(self._h))

    @property
    def path(self) -> str:
        """'split' (nominal / Riccati / forward kernels) or 'fused' (one kernel)."""
        return 'split' if self.lib.mpcb_path(self._h) == 1 else 'fused'

    def set_timing(self, enable: bool = True):
        """Record HIP events around each kernel phase of later solves (see ``last_timing``)."""
        _lib.check(self.lib.mpcb_set_timing(self._h, 1 if enable else 0))

    def last_timing(self) -> dict:
        """Device ms of the last timed solve's phases: nominal, riccati (dominant), forward
        (17/6 model: nominal, riccati = Riccati + forward or the interior point, linearise)."""
        ms = (ctypes.c_float * 3)()
        _lib.check(self.lib.mpcb_last_timing(self._h, ms))
        if self.nx == 17:
            return dict(nominal=ms[0], riccati=ms[1], linearise=ms[2])
        return dict(nominal=ms[0], riccati=ms[1], forward=ms[2])

    def last_kernels(self) -> dict:
        """{phase: rocprof kernel name} of what the last solve launched (phases as ``last_timing``)."""
        return _lib.kernel_names(lambda b, n: self.lib.mpcb_last_kernels(self._h, b, n), self.nx == 17)

    def plan_kernels(self, B: int, iterate: bool = False, want_traj: bool = True) -> dict:
        """{phase: rocprof kernel name} a solve of B instances launches on this handle's config."""
        return _lib.plan_kernels(self._c, self.max_batch, B, iterate, want_traj)

    def _dev(self, t, shape_tail, name, batch=None, allow_broadcast=False):
        """Coerce to a contiguous device tensor of the handle dtype; return (tensor, stride)."""
        torch = _torch()
        if isinstance(t, np.ndarray) and not t.flags.writeable:
            t = t.copy()   # torch.as_tensor warns on read-only arrays
        t = torch.as_tensor(t, dtype=self.dtype, device=self._tdev)
        if t.dim() == len(shape_tail):
            t = t.unsqueeze(0)
        if tuple(t.shape[1:]) != tuple(shape_tail):
            raise ValueError(f'{name}: expected shape [B, {", ".join(map(str, shape_tail))}], '
                             f'got {tuple(t.shape)}')
        t = t.contiguous()
        n = math.prod(shape_tail)
        if batch is not None and t.shape[0] != batch:
            if allow_broadcast and t.shape[0] == 1:
                return t, 0
            raise ValueError(f'{name}: batch {t.shape[0]} != {batch}')
        return t, n

    def _stream(self):
        return ctypes.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def _outputs(self, B, want_traj):
        """Fresh (u0, X, U, status) for a solve.  The caller installs them as the handle's last
        solve only once the library has accepted the call, so a refused solve leaves
        ``get_control()`` and the others at the previous solve's tensors."""
        torch = _torch()
        dev = self._tdev
        N = self.cfg.N
        u0 = torch.empty((B, self.nu), dtype=self.dtype, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        X = U = None
        if want_traj:
            X = torch.empty((B, N + 1, self.nx), dtype=self.dtype, device=dev)
            U = torch.empty((B, N, self.nu), dtype=self.dtype, device=dev)
        return u0, X, U, status

    @staticmethod
    def _ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)

    def _pw_weights(self, B, Q, R, QN, full=False):
        """Per-instance weight arguments as device matrices: a list of (tensor or None, stride) for
        Q, R, QN.  A weight always carries a batch axis: 2-D [B|1, n] holds diagonals, 3-D
        [B|1, n, n] matrices, which are passed as 0.5 (M + M^T).  Built on the device: no host read,
        no synchronisation.  ``full``: the caller is one of the 17/6 entries (``*_pw17``)."""
        torch = _torch()
        if self.nx == 17 and not full:
            raise ValueError('per-instance weights cover the 12/4 model only')
        if self.nx != 17 and full:
            raise ValueError('the pw17 entries cover the 17/6 model (12/4: the Q, R, QN keywords of solve_iterate)')
        out = []
        for name, w, n in (('Q', Q, self.nx), ('R', R, self.nu), ('QN', QN, self.nx)):
            if w is None:
                out.append((None, 0))
                continue
            if isinstance(w, np.ndarray) and not w.flags.writeable:
                w = w.copy()   # torch.as_tensor warns on read-only arrays
            t = torch.as_tensor(w, dtype=self.dtype, device=self._tdev)
            if t.dim() == 2 and t.shape[1] == n:
                t = torch.diag_embed(t)
            elif t.dim() == 3 and tuple(t.shape[1:]) == (n, n):
                t = 0.5 * (t + t.transpose(1, 2))
            else:
                raise ValueError(f'{name}: expected [B|1, {n}] (diagonals) or [B|1, {n}, {n}], got {tuple(t.shape)}')
            if t.shape[0] != B and t.shape[0] != 1:
                raise ValueError(f'{name}: batch {t.shape[0]} != {B}')
            out.append((t.contiguous(), 0 if t.shape[0] == 1 else n * n))
        return out

    def _model_arg(self, model, B):
        """A ``model=`` argument as (device tensor, stride): vehicle records [B|1, 14] or [14]
        (mpcb.h MPCB_MODEL_REC); wider rows are padding that the library never reads."""
        torch = _torch()
        if self.nx == 17:
            raise ValueError('per-instance models cover the 12/4 model only (17/6: set_params)')
        if isinstance(model, np.ndarray) and not model.flags.writeable:
            model = model.copy()   # torch.as_tensor warns on read-only arrays
        t = torch.as_tensor(model, dtype=self.dtype, device=self._tdev)
        if t.dim() == 1:
            t = t.unsqueeze(0)
        if t.dim() != 2 or t.shape[1] < _lib.MODEL_REC:
            raise ValueError(f'model: expected [B|1, {_lib.MODEL_REC}] (or wider, padded rows), got {tuple(t.shape)}')
        if t.shape[0] != B and t.shape[0] != 1:
            raise ValueError(f'model: batch {t.shape[0]} != {B}')
        t = t.contiguous()
        return t, 0 if t.shape[0] == 1 else t.shape[1]

    def pack_model(self, B=None, mass=None, J=None, lx=None, ly=None, c=None, t_blast=None):
        """Vehicle records for ``sim_step`` / ``solve_iterate`` / ``solve_iterate_gains`` /
        ``closed_loop`` (12/4 model; mpcb.h MPCB_MODEL_REC): a [B|1, 14] device tensor of the
        handle's dtype, row = [mass, lx, ly, c, t_blast, J row-major].  Each scalar field is a
        number, [B] or [1]; ``J`` is [3,3] (one matrix), [B,3,3] or [B,3] (diagonals; a [3,3]
        argument is always one matrix).  An omitted field takes the handle's config value (the
        current T_blast of ``set_t_blast``).  ``B`` None: the largest batch among the fields.
        Built on the device: no host read-back, no synchronisation.  mass > 0 and a symmetric
        positive definite J are the caller's contract."""
        torch = _torch()
        if self.nx == 17:
            raise ValueError('per-instance models cover the 12/4 model only (17/6: set_params)')
        cols = []
        for name, v in (('mass', mass), ('lx', lx), ('ly', ly), ('c', c), ('t_blast', t_blast)):
            if isinstance(v, np.ndarray) and not v.flags.writeable:
                v = v.copy()   # torch.as_tensor warns on read-only arrays
            t = torch.as_tensor(getattr(self.cfg, name) if v is None else v, dtype=self.dtype, device=self._tdev)
            if t.dim() > 1:
                raise ValueError(f'{name}: expected a scalar, [B] or [1], got {tuple(t.shape)}')
            cols.append(t.reshape(-1, 1))
        if J is None:
            J = np.asarray(self.cfg.J, dtype=np.float64).reshape(3, 3).copy()
        elif isinstance(J, np.ndarray) and not J.flags.writeable:
            J = J.copy()
        Jt = torch.as_tensor(J, dtype=self.dtype, device=self._tdev)
        if tuple(Jt.shape) == (3, 3):
            Jt = Jt.reshape(1, 9)
        elif Jt.dim() == 3 and tuple(Jt.shape[1:]) == (3, 3):
            Jt = Jt.reshape(-1, 9)
        elif Jt.dim() == 2 and Jt.shape[1] == 3:
            Jt = torch.diag_embed(Jt).reshape(-1, 9)
        else:
            raise ValueError(f'J: expected [3, 3], [B, 3, 3] or [B, 3] (diagonals), got {tuple(Jt.shape)}')
        cols.append(Jt)
        rows = max(t.shape[0] for t in cols) if B is None else int(B)
        for name, t in zip(('mass', 'lx', 'ly', 'c', 't_blast', 'J'), cols):
            if t.shape[0] != rows and t.shape[0] != 1:
                raise ValueError(f'{name}: batch {t.shape[0]} != {rows}')
        return torch.cat([t.expand(rows, t.shape[1]) for t in cols], dim=1).contiguous()

    # ------------------------------------------------------------------ API
    def solve(self, x0, x_ref, u_ref, wind=None, want_traj: bool = True, out=None):
        """One SQP_RTI step per instance, linearised at the RK4 rollout of u_ref from x0.

        x0 [B,12]; x_ref [B|1,N+1,12]; u_ref [B|1,N,4]; wind [B|1,3] (optional).
        Returns the first-step controls u0* [B,4] (device tensor, async).
        """
        N = self.cfg.N
        x0, _ = self._dev(x0, (self.nx,), 'x0')
        B = x0.shape[0]
        if B > self.max_batch:
            raise ValueError(f'batch {B} > max_batch {self.max_batch}')
        xr, xr_sb = self._dev(x_ref, (N + 1, self.nx), 'x_ref', B, allow_broadcast=True)
        ur, ur_sb = self._dev(u_ref, (N, self.nu), 'u_ref', B, allow_broadcast=True)
        wd, wd_sb = (None, 0) if wind is None else self._dev(wind, (3,), 'wind', B, allow_broadcast=True)
        u0, X, U, status = self._outputs(B, want_traj) if out is None else out
        keep = (x0, xr, ur, wd)
        _lib.check(self.lib.mpcb_solve(
            self._h, B, self._ptr(x0), self.nx, self._ptr(xr), xr_sb, self._ptr(ur), ur_sb,
            self._ptr(wd), wd_sb, self._ptr(u0), self._ptr(X), self._ptr(U), self._ptr(status), self._stream()))
        self._keep = keep
        self._u0, self._X, self._U, self._status = u0, X, U, status
        return self._u0

    def solve_iterate(self, x0, xbar, ubar, x_ref, u_ref, wind=None, out=None, Q=None, R=None, QN=None,
                      model=None):
        """acados SQP_RTI step from the persistent iterate (xbar [B,N+1,12], ubar [B,N,4]).

        ``Q``, ``R``, ``QN``: cost weights per instance (mpcb_solve_iterate_pw; 12/4 model, fp64
        with the input box).  Each carries a batch axis: 2-D ``[B|1, n]`` holds diagonals, 3-D
        ``[B|1, n, n]`` symmetric matrices (passed as 0.5 (M + M^T)); None = the handle's matrix.
        Any of them routes the call to that entry point, whose input box is the plain active set
        (status 2 at its cap, no interior-point fallback; ``qp_stats`` is not updated); with all
        three None the call is the shared-weight solve.

        ``model``: a vehicle per instance (mpcb_solve_iterate_pm; 12/4 model): records [B|1, 14]
        as ``pack_model`` builds them (or wider, padded rows), an array or a tensor.  It combines
        with ``Q``, ``R``, ``QN`` and has that entry point's input box and refusals; with
        ``model=None`` the call takes the path it takes without the keyword."""
        N = self.cfg.N
        x0, _ = self._dev(x0, (self.nx,), 'x0')
        B = x0.shape[0]
        xb, _ = self._dev(xbar, (N + 1, self.nx), 'xbar', B)
        ub, _ = self._dev(ubar, (N, self.nu), 'ubar', B)
        xr, xr_sb = self._dev(x_ref, (N + 1, self.nx), 'x_ref', B, allow_broadcast=True)
        ur, ur_sb = self._dev(u_ref, (N, self.nu), 'u_ref', B, allow_broadcast=True)
        wd, wd_sb = (None, 0) if wind is None else self._dev(wind, (3,), 'wind', B, allow_broadcast=True)
        u0, X, U, status = self._outputs(B, True) if out is None else out
        if model is not None:
            if B > self.max_batch:
                raise ValueError(f'batch {B} > max_batch {self.max_batch}')
            md, m_sb = self._model_arg(model, B)
            (Qd, Q_sb), (Rd, R_sb), (QNd, QN_sb) = self._pw_weights(B, Q, R, QN)
            _lib.check(self.lib.mpcb_solve_iterate_pm(
                self._h, B, self._ptr(x0), self.nx, self._ptr(xb), self._ptr(ub), self._ptr(xr), xr_sb,
                self._ptr(ur), ur_sb, self._ptr(wd), wd_sb, self._ptr(Qd), Q_sb, self._ptr(Rd), R_sb,
                self._ptr(QNd), QN_sb, self._ptr(md), m_sb, self._ptr(u0), self._ptr(X), self._ptr(U),
                self._ptr(status), self._stream()))
            self._keep = (x0, xb, ub, xr, ur, wd, Qd, Rd, QNd, md)
            self._u0, self._X, self._U, self._status = u0, X, U, status
            return self._u0
        if Q is not None or R is not None or QN is not None:
            if B > self.max_batch:
                raise ValueError(f'batch {B} > max_batch {self.max_batch}')
            (Qd, Q_sb), (Rd, R_sb), (QNd, QN_sb) = self._pw_weights(B, Q, R, QN)
            _lib.check(self.lib.mpcb_solve_iterate_pw(
                self._h, B, self._ptr(x0), self.nx, self._ptr(xb), self._ptr(ub), self._ptr(xr), xr_sb,
                self._ptr(ur), ur_sb, self._ptr(wd), wd_sb, self._ptr(Qd), Q_sb, self._ptr(Rd), R_sb,
                self._ptr(QNd), QN_sb, self._ptr(u0), self._ptr(X), self._ptr(U), self._ptr(status),
                self._stream()))
            self._keep = (x0, xb, ub, xr, ur, wd, Qd, Rd, QNd)
            self._u0, self._X, self._U, self._status = u0, X, U, status
            return self._u0
        _lib.check(self.lib.mpcb_solve_iterate(
            self._h, B, self._ptr(x0), self.nx, self._ptr(xb), self._ptr(ub), self._ptr(xr), xr_sb,
            self._ptr(ur), ur_sb, self._ptr(wd), wd_sb, self._ptr(u0), self._ptr(X), self._ptr(U),
            self._ptr(status), self._stream()))
        self._keep = (x0, xb, ub, xr, ur, wd)
        self._u0, self._X, self._U, self._status = u0, X, U, status
        return self._u0

    def solve_iterate_pw17(self, x0, xbar, ubar, x_ref, u_ref, Q=None, R=None, QN=None, out=None):
        """``solve_iterate`` on a 17/6 handle with the cost weights given per instance
        (mpcb_solve_iterate_pw17): ``Q`` [B|1,17] or [B|1,17,17], ``R`` [B|1,6] or [B|1,6,6], ``QN``
        like Q, by the shape rule of ``solve_iterate`` (2-D = diagonals, 3-D = matrices, passed as
        0.5 (M + M^T)); None = the handle's matrix.  Parameters, boxes and ``max_as_iter`` are the
        handle's; both dtypes and every box mode.  Built on the device, no synchronisation;
        ``qp_stats``, ``last_kernels`` and ``last_timing`` do not see the call.  With all three None
        it returns the bits of ``solve_iterate``.  ``ValueError`` on a 12/4 handle."""
        if self.nx != 17:
            raise ValueError('solve_iterate_pw17 covers the 17/6 model (12/4: the Q, R, QN keywords of solve_iterate)')
        N = self.cfg.N
        x0, _ = self._dev(x0, (self.nx,), 'x0')
        B = x0.shape[0]
        if B > self.max_batch:
            raise ValueError(f'batch {B} > max_batch {self.max_batch}')
        xb, _ = self._dev(xbar, (N + 1, self.nx), 'xbar', B)
        ub, _ = self._dev(ubar, (N, self.nu), 'ubar', B)
        xr, xr_sb = self._dev(x_ref, (N + 1, self.nx), 'x_ref', B, allow_broadcast=True)
        ur, ur_sb = self._dev(u_ref, (N, self.nu), 'u_ref', B, allow_broadcast=True)
        u0, X, U, status = self._outputs(B, True) if out is None else out
        (Qd, Q_sb), (Rd, R_sb), (QNd, QN_sb) = self._pw_weights(B, Q, R, QN, full=True)
        _lib.check(self.lib.mpcb_solve_iterate_pw17(
            self._h, B, self._ptr(x0), self.nx, self._ptr(xb), self._ptr(ub), self._ptr(xr), xr_sb,
            self._ptr(ur), ur_sb, self._ptr(Qd), Q_sb, self._ptr(Rd), R_sb, self._ptr(QNd), QN_sb,
            self._ptr(u0), self._ptr(X), self._ptr(U), self._ptr(status), self._stream()))
        self._keep = (x0, xb, ub, xr, ur, Qd, Rd, QNd)
        self._u0, self._X, self._U, self._status = u0, X, U, status
        return self._u0

    def solve_iterate_vjp_pw17(self, xbar, ubar, gX=None, gU=None, U=None, X=None, x_ref=None, u_ref=None,
                               weights=False, fixed=None, active_tol=None, Q=None, R=None, QN=None,
                               fixed_x=None, state_active_tol=None):
        """``solve_iterate_vjp`` on a 17/6 handle at the per-instance weights a ``solve_iterate_pw17``
        step was given (mpcb_solve_vjp_pw17): the product and, with ``weights=True``, gQ [B,17,17],
        gR [B,6,6], gQN [B,17,17] at instance b's matrices, each instance's own (no batch sum).
        The mask rules (``fixed``, or ``U`` with ``active_tol``) are those of the 17/6 branch of
        ``solve_iterate_vjp``; ``Q``, ``R``, ``QN`` follow ``solve_iterate_pw17``.  ``fixed_x`` /
        ``state_active_tol``: the active state rows, as in ``solve_iterate_vjp`` (mpcb_solve_vjp17_sx
        with the weight arguments).  ``ValueError`` on a 12/4 handle; without the state-row arguments
        a state-box handle is refused by the library."""
        if self.nx != 17:
            raise ValueError('solve_iterate_vjp_pw17 covers the 17/6 model (12/4: the Q, R, QN keywords of '
                             'solve_iterate_vjp)')
        return self._solve_iterate_vjp17(xbar, ubar, gX, gU, U, None, X, x_ref, u_ref, weights, fixed,
                                         active_tol, pw=(Q, R, QN), fixed_x=fixed_x,
                                         state_active_tol=state_active_tol)

    def evaluate(self, X, U, x_ref, u_ref, x0=None, wind=None, stat=True):
        """Cost and KKT residuals of the iterate (X [B,N+1,nx], U [B,N,nu]) per instance
        (mpcb_eval; acados ``get_cost()`` / ``get_residuals()``): a dict of [B] device tensors
        ``cost``, ``res_eq`` (dynamics defect; with ``x0`` also |x_0 - x0|), ``res_ineq`` (box
        violation) and, unless ``stat=False``, ``res_stat`` (natural residual of the reduced
        gradient; needs the adjoint sweep, unsupported with the state box).  Asynchronous, like
        ``solve``."""
        torch = _torch()
        N = self.cfg.N
        Xd, _ = self._dev(X, (N + 1, self.nx), 'X')
        B = Xd.shape[0]
        if B > self.max_batch:
            raise ValueError(f'batch {B} > max_batch {self.max_batch}')
        Ud, _ = self._dev(U, (N, self.nu), 'U', B)
        xr, xr_sb = self._dev(x_ref, (N + 1, self.nx), 'x_ref', B, allow_broadcast=True)
        ur, ur_sb = self._dev(u_ref, (N, self.nu), 'u_ref', B, allow_broadcast=True)
        x0d, x0_sb = (None, 0) if x0 is None else self._dev(x0, (self.nx,), 'x0', B)
        wd, wd_sb = (None, 0) if wind is None else self._dev(wind, (3,), 'wind', B, allow_broadcast=True)
        out = {k: torch.empty((B,), dtype=self.dtype, device=self._tdev)
               for k in ('cost', 'res_eq', 'res_ineq') + (('res_stat',) if stat else ())}
        self._keep_eval = (Xd, Ud, xr, ur, x0d, wd)
        _lib.check(self.lib.mpcb_eval(
            self._h, B, self._ptr(x0d), x0_sb, self._ptr(Xd), self._ptr(Ud), self._ptr(xr), xr_sb,
            self._ptr(ur), ur_sb, self._ptr(wd), wd_sb, self._ptr(out['cost']), self._ptr(out['res_eq']),
            self._ptr(out['res_ineq']), self._ptr(out.get('res_stat')), self._stream()))
        return out

    def solve_iterate_vjp(self, xbar, ubar, gX=None, gU=None, U=None, wind=None, X=None, x_ref=None,
                          u_ref=None, weights=False, fixed=None, active_tol=None, Q=None, R=None, QN=None,
                          fixed_x=None, state_active_tol=None):
        """Vector-Jacobian product of ``solve_iterate`` (mpcb_solve_vjp; 17/6: below): with J the
        Jacobian of (X, U) with respect to (x0, x_ref, u_ref) at fixed xbar, ubar, wind, weights
        and active set, returns J^T (gX, gU) as a dict of device tensors ``gx0`` [B,12],
        ``gxref`` [B,N+1,12], ``guref`` [B,N,4] and ``status`` [B] (int32).  ``gX`` [B,N+1,12] and
        ``gU`` [B,N,4] are the cotangents (one may be None = 0; add a cotangent of u0 to
        ``gU[:, 0]``).  ``U`` [B,N,4] is the solve's output, read for the active set: required on
        an input-box handle.  Per-instance gradients: sum ``gxref`` / ``guref`` over the batch for
        a reference that was broadcast.  Asynchronous, like ``evaluate``.

        ``weights=True`` (mpcb_solve_vjp_w, the same launch) adds the gradients with respect to
        the cost weights, per instance: ``gQ`` [B,12,12], ``gR`` [B,4,4], ``gQN`` [B,12,12],
        symmetric; for a symmetric perturbation dQ the loss changes by <gQ.sum(0), dQ>.  It needs
        the solve's output ``X`` [B,N+1,12] and ``U`` and its references ``x_ref`` [B|1,N+1,12],
        ``u_ref`` [B|1,N,4] (include/mpcb.h has the formula).

        ``Q``, ``R``, ``QN`` (12/4): the per-instance weights the solve was given, by the shape
        rule of ``solve_iterate`` (mpcb_solve_vjp_pw, both dtypes, with and without the box); the
        product and, with ``weights=True``, gQ, gR, gQN are then taken at instance b's matrices,
        and the weight gradients are each instance's own (no batch sum).

        On a 17/6 handle (mpcb_solve_vjp17; shapes with 17 and 6) the active set is an argument,
        because the interior point leaves U near its bounds and not on them: ``fixed`` is a
        bool / uint8 tensor [B,N,6], nonzero = clamped.  Without it, and with ``U`` on an input-box
        handle, the mask is ``(U <= lbu + active_tol) | (U >= ubu - active_tol)``; ``active_tol``
        defaults to 1e-6 on an f64 handle (the tolerance the oracle's KKT certificate calls a
        component active at) and has no default on an f32 handle, whose interior point stops near
        mu = 1e-6: omitting it there raises ``ValueError``.  Without ``fixed`` and ``U`` nothing is
        clamped.  The mask used is returned as ``fixed``.  ``wind`` raises as in ``solve_iterate``.

        The 17/6 state box (mpcb_solve_vjp17_sx, f64).  ``fixed_x`` is a bool / uint8 tensor
        [B,N+1,17], nonzero = state row (k, i) is active (stages 0 and N are never read): the product
        then holds dx_k[i] = 0 on those rows, exact for the masks it is given on any f64 17/6 handle.
        Without it, ``state_active_tol`` with ``X`` (the solve's output) on a state-box handle builds
        the mask by ``active_mask17x``.  Either way the masks used are returned as ``fixed`` and
        ``fixed_x``, and ``status`` may be 2 (MPCB_STATUS_MAXITER): the rows are (nearly) dependent,
        the solve is not differentiable there, and the outputs are the last pass's.  Without both
        arguments a handle with the state box is refused, as before."""
        pw = Q is not None or R is not None or QN is not None
        if self.nx == 17:
            if pw:
                raise ValueError('per-instance weights cover the 12/4 model only')
            return self._solve_iterate_vjp17(xbar, ubar, gX, gU, U, wind, X, x_ref, u_ref, weights, fixed,
                                             active_tol, fixed_x=fixed_x, state_active_tol=state_active_tol)
        if fixed_x is not None or state_active_tol is not None:
            raise ValueError('fixed_x / state_active_tol belong to the 17/6 model')
        if fixed is not None or active_tol is not None:
            raise ValueError('fixed / active_tol belong to the 17/6 model: the 12/4 product reads its active '
                             'set from U')
        torch = _torch()
        N = self.cfg.N
        xb, _ = self._dev(xbar, (N + 1, self.nx), 'xbar')
        B = xb.shape[0]
        if B > self.max_batch:
            raise ValueError(f'batch {B} > max_batch {self.max_batch}')
        ub, _ = self._dev(ubar, (N, self.nu), 'ubar', B)
        gXd = None if gX is None else self._dev(gX, (N + 1, self.nx), 'gX', B)[0]
        gUd = None if gU is None else self._dev(gU, (N, self.nu), 'gU', B)[0]
        Ud = None if U is None else self._dev(U, (N, self.nu), 'U', B)[0]
        wd, wd_sb = (None, 0) if wind is None else self._dev(wind, (3,), 'wind', B, allow_broadcast=True)
        dev = self._tdev
        out = dict(gx0=torch.empty((B, self.nx), dtype=self.dtype, device=dev),
                   gxref=torch.empty((B, N + 1, self.nx), dtype=self.dtype, device=dev),
                   guref=torch.empty((B, N, self.nu), dtype=self.dtype, device=dev),
                   status=torch.empty((B,), dtype=torch.int32, device=dev))
        Xd = xr = ur = None
        xr_sb = ur_sb = 0
        if weights:
            if X is None or U is None or x_ref is None or u_ref is None:
                raise ValueError('weights=True needs X, U, x_ref and u_ref of the solve')
            Xd, _ = self._dev(X, (N + 1, self.nx), 'X', B)
            xr, xr_sb = self._dev(x_ref, (N + 1, self.nx), 'x_ref', B, allow_broadcast=True)
            ur, ur_sb = self._dev(u_ref, (N, self.nu), 'u_ref', B, allow_broadcast=True)
            out.update(gQ=torch.empty((B, self.nx, self.nx), dtype=self.dtype, device=dev),
                       gR=torch.empty((B, self.nu, self.nu), dtype=self.dtype, device=dev),
                       gQN=torch.empty((B, self.nx, self.nx), dtype=self.dtype, device=dev))
        if pw:
            (Qd, Q_sb), (Rd, R_sb), (QNd, QN_sb) = self._pw_weights(B, Q, R, QN)
            self._keep_vjp = (xb, ub, gXd, gUd, Ud, wd, Xd, xr, ur, Qd, Rd, QNd)
            _lib.check(self.lib.mpcb_solve_vjp_pw(
                self._h, B, self._ptr(xb), self._ptr(ub), self._ptr(Xd), self._ptr(Ud), self._ptr(xr), xr_sb,
                self._ptr(ur), ur_sb, self._ptr(wd), wd_sb, self._ptr(Qd), Q_sb, self._ptr(Rd), R_sb,
                self._ptr(QNd), QN_sb, self._ptr(gXd), self._ptr(gUd), self._ptr(out['gx0']),
                self._ptr(out['gxref']), self._ptr(out['guref']), self._ptr(out.get('gQ')),
                self._ptr(out.get('gR')), self._ptr(out.get('gQN')), self._ptr(out['status']), self._stream()))
            return out
        if weights:
            self._keep_vjp = (xb, ub, gXd, gUd, Ud, wd, Xd, xr, ur)
            _lib.check(self.lib.mpcb_solve_vjp_w(
                self._h, B, self._ptr(xb), self._ptr(ub), self._ptr(Xd), self._ptr(Ud), self._ptr(xr), xr_sb,
                self._ptr(ur), ur_sb, self._ptr(wd), wd_sb, self._ptr(gXd), self._ptr(gUd),
                self._ptr(out['gx0']), self._ptr(out['gxref']), self._ptr(out['guref']), self._ptr(out['gQ']),
                self._ptr(out['gR']), self._ptr(out['gQN']), self._ptr(out['status']), self._stream()))
            return out
        self._keep_vjp = (xb, ub, gXd, gUd, Ud, wd)
        _lib.check(self.lib.mpcb_solve_vjp(
            self._h, B, self._ptr(xb), self._ptr(ub), self._ptr(Ud), self._ptr(wd), wd_sb,
            self._ptr(gXd), self._ptr(gUd), self._ptr(out['gx0']), self._ptr(out['gxref']),
            self._ptr(out['guref']), self._ptr(out['status']), self._stream()))
        return out

    def active_mask17(self, U, active_tol=None):
        """The 17/6 active set of ``U`` [B,N,6] by tolerance: a uint8 tensor, 1 where
        ``U <= lbu + active_tol`` or ``U >= ubu - active_tol`` (``solve_iterate_vjp`` has the
        default and why an f32 handle has none); None on a handle without the input box."""
        if not self.cfg.boxed:
            return None
        if active_tol is None:
            if self.cfg.dtype != 'f64':
                raise ValueError('active_tol is required on an f32 17/6 handle: its interior point stops near '
                                 'mu = 1e-6, so no fixed number separates active from inactive components')
            active_tol = 1e-6
        torch = _torch()
        lb = torch.as_tensor(np.broadcast_to(np.asarray(self.cfg.lbu, dtype=np.float64), (self.nu,)).copy(),
                             dtype=self.dtype, device=self._tdev)
        ub = torch.as_tensor(np.broadcast_to(np.asarray(self.cfg.ubu, dtype=np.float64), (self.nu,)).copy(),
                             dtype=self.dtype, device=self._tdev)
        return ((U <= lb + active_tol) | (U >= ub - active_tol)).to(torch.uint8).contiguous()

    def active_mask17x(self, X, state_active_tol=None):
        """The active state rows of ``X`` [B,N+1,17] by tolerance on a 17/6 state-box handle: a uint8
        tensor [B,N+1,17], 1 where ``X <= lbx + state_active_tol`` or ``X >= ubx - state_active_tol`` on
        stages 1..N-1 (the rows the solver constrains), 0 on stages 0 and N.  The default is 1e-6, the
        tolerance of the reference's KKT certificate; the solver's polish leaves an active row within
        1e-10 of its bound.  None on a handle without the state box."""
        if self.cfg.lbx is None:
            return None
        if state_active_tol is None:
            state_active_tol = 1e-6
        torch = _torch()
        lb = torch.as_tensor(np.broadcast_to(np.asarray(self.cfg.lbx, dtype=np.float64), (self.nx,)).copy(),
                             dtype=self.dtype, device=self._tdev)
        ub = torch.as_tensor(np.broadcast_to(np.asarray(self.cfg.ubx, dtype=np.float64), (self.nx,)).copy(),
                             dtype=self.dtype, device=self._tdev)
        m = ((X <= lb + state_active_tol) | (X >= ub - state_active_tol)).to(torch.uint8)
        m[:, 0] = 0
        m[:, -1] = 0
        return m.contiguous()

    def active_mask(self, U, active_tol=None):
        """The active set of ``U`` [B,N,nu] by tolerance on either model (``active_mask17``'s rule
        and defaults; that name is kept for the 17/6 callers)."""
        return self.active_mask17(U, active_tol)

    def _solve_iterate_vjp17(self, xbar, ubar, gX, gU, U, wind, X, x_ref, u_ref, weights, fixed, active_tol,
                             pw=None, fixed_x=None, state_active_tol=None):
        torch = _torch()
        if wind is not None:
            raise _lib.MpcbError('mpcb error -4: wind is a 12/4-model extension')
        N = self.cfg.N
        xb, _ = self._dev(xbar, (N + 1, self.nx), 'xbar')
        B = xb.shape[0]
        if B > self.max_batch:
            raise ValueError(f'batch {B} > max_batch {self.max_batch}')
        ub, _ = self._dev(ubar, (N, self.nu), 'ubar', B)
        gXd = None if gX is None else self._dev(gX, (N + 1, self.nx), 'gX', B)[0]
        gUd = None if gU is None else self._dev(gU, (N, self.nu), 'gU', B)[0]
        Ud = None if U is None else self._dev(U, (N, self.nu), 'U', B)[0]
        dev = self._tdev
        if fixed is not None:
            if isinstance(fixed, np.ndarray) and not fixed.flags.writeable:
                fixed = fixed.copy()   # torch.as_tensor warns on read-only arrays
            fx = torch.as_tensor(fixed, device=dev)
            if tuple(fx.shape) != (B, N, self.nu):
                raise ValueError(f'fixed: expected shape [{B}, {N}, {self.nu}], got {tuple(fx.shape)}')
            fx = (fx != 0).to(torch.uint8).contiguous()
        elif Ud is not None:
            fx = self.active_mask17(Ud, active_tol)
        else:
            fx = None
        # the active state rows (mpcb_solve_vjp17_sx): given, or by tolerance from the solve's X
        fxx = None
        if fixed_x is not None:
            if isinstance(fixed_x, np.ndarray) and not fixed_x.flags.writeable:
                fixed_x = fixed_x.copy()
            fxx = torch.as_tensor(fixed_x, device=dev)
            if tuple(fxx.shape) != (B, N + 1, self.nx):
                raise ValueError(f'fixed_x: expected shape [{B}, {N + 1}, {self.nx}], got {tuple(fxx.shape)}')
            fxx = (fxx != 0).to(torch.uint8).contiguous()
        elif state_active_tol is not None:
            if X is None:
                raise ValueError('state_active_tol needs X (the solve\'s output) to build the mask from')
            fxx = self.active_mask17x(self._dev(X, (N + 1, self.nx), 'X', B)[0], state_active_tol)
        out = dict(gx0=torch.empty((B, self.nx), dtype=self.dtype, device=dev),
                   gxref=torch.empty((B, N + 1, self.nx), dtype=self.dtype, device=dev),
                   guref=torch.empty((B, N, self.nu), dtype=self.dtype, device=dev),
                   status=torch.empty((B,), dtype=torch.int32, device=dev), fixed=fx)
        Xd = xr = ur = None
        xr_sb = ur_sb = 0
        if weights:
            if X is None or U is None or x_ref is None or u_ref is None:
                raise ValueError('weights=True needs X, U, x_ref and u_ref of the solve')
            Xd, _ = self._dev(X, (N + 1, self.nx), 'X', B)
            xr, xr_sb = self._dev(x_ref, (N + 1, self.nx), 'x_ref', B, allow_broadcast=True)
            ur, ur_sb = self._dev(u_ref, (N, self.nu), 'u_ref', B, allow_broadcast=True)
            out.update(gQ=torch.empty((B, self.nx, self.nx), dtype=self.dtype, device=dev),
                       gR=torch.empty((B, self.nu, self.nu), dtype=self.dtype, device=dev),
                       gQN=torch.empty((B, self.nx, self.nx), dtype=self.dtype, device=dev))
        if fxx is not None:   # (the weights as arguments, or all NULL: the handle's)
            (Qd, Q_sb), (Rd, R_sb), (QNd, QN_sb) = ((None, 0),) * 3 if pw is None else \
                self._pw_weights(B, *pw, full=True)
            out['fixed_x'] = fxx
            self._keep_vjp = (xb, ub, gXd, gUd, Ud, fx, fxx, Xd, xr, ur, Qd, Rd, QNd)
            _lib.check(self.lib.mpcb_solve_vjp17_sx(
                self._h, B, self._ptr(xb), self._ptr(ub), self._ptr(fx), self._ptr(fxx), self._ptr(Xd),
                self._ptr(Ud if weights else None), self._ptr(xr), xr_sb, self._ptr(ur), ur_sb,
                self._ptr(Qd), Q_sb, self._ptr(Rd), R_sb, self._ptr(QNd), QN_sb,
                self._ptr(gXd), self._ptr(gUd), self._ptr(out['gx0']), self._ptr(out['gxref']),
                self._ptr(out['guref']), self._ptr(out.get('gQ')), self._ptr(out.get('gR')),
                self._ptr(out.get('gQN')), self._ptr(out['status']), self._stream()))
            return out
        if pw is not None:   # (solve_iterate_vjp_pw17: the weights as arguments)
            (Qd, Q_sb), (Rd, R_sb), (QNd, QN_sb) = self._pw_weights(B, *pw, full=True)
            self._keep_vjp = (xb, ub, gXd, gUd, Ud, fx, Xd, xr, ur, Qd, Rd, QNd)
            _lib.check(self.lib.mpcb_solve_vjp_pw17(
                self._h, B, self._ptr(xb), self._ptr(ub), self._ptr(fx), self._ptr(Xd),
                self._ptr(Ud if weights else None), self._ptr(xr), xr_sb, self._ptr(ur), ur_sb,
                self._ptr(Qd), Q_sb, self._ptr(Rd), R_sb, self._ptr(QNd), QN_sb,
                self._ptr(gXd), self._ptr(gUd), self._ptr(out['gx0']), self._ptr(out['gxref']),
                self._ptr(out['guref']), self._ptr(out.get('gQ')), self._ptr(out.get('gR')),
                self._ptr(out.get('gQN')), self._ptr(out['status']), self._stream()))
            return out
        self._keep_vjp = (xb, ub, gXd, gUd, Ud, fx, Xd, xr, ur)
        _lib.check(self.lib.mpcb_solve_vjp17(
            self._h, B, self._ptr(xb), self._ptr(ub), self._ptr(fx), self._ptr(Xd),
            self._ptr(Ud if weights else None), self._ptr(xr), xr_sb, self._ptr(ur), ur_sb,
            self._ptr(gXd), self._ptr(gUd), self._ptr(out['gx0']), self._ptr(out['gxref']),
            self._ptr(out['guref']), self._ptr(out.get('gQ')), self._ptr(out.get('gR')),
            self._ptr(out.get('gQN')), self._ptr(out['status']), self._stream()))
        return out

    def solve_iterate_gains(self, xbar, ubar, U=None, fixed=None, active_tol=None, wind=None,
                            want_K=True, want_P0=True, model=None):
        """Feedback gains and cost-to-go Hessian of the ``solve_iterate`` step at (xbar, ubar)
        (mpcb_solve_gains; include/mpcb.h has the recursion): a dict of device tensors ``K``
        [B,N,nu,nx] (``U'_k - U_k = K_k (X'_k - X_k)`` between two solves that differ in x0 on one
        active set; ``K[:, 0]`` is du0/dx0), ``P0`` [B,nx,nx] (the Hessian of the QP's optimal
        value in x0, bitwise symmetric), ``status`` [B] (int32) and ``fixed``, the mask used (None
        where the library read the set from ``U`` or nothing is clamped).  ``want_K`` /
        ``want_P0`` = False leaves that output out (None), not both.  Asynchronous.

        The active set.  ``fixed`` is a bool / uint8 tensor [B,N,nu], nonzero = clamped, on both
        models.  Without it, ``active_tol`` with ``U`` builds the mask
        ``(U <= lbu + active_tol) | (U >= ubu - active_tol)`` on an input-box handle; on a 12/4
        input-box handle ``U`` alone has the library read the set by the rule of
        ``solve_iterate_vjp`` (on or beyond a bound; required there when there is no mask), which
        misses an instance the active set handed to the interior point: a tolerance finds it.  On
        17/6 ``U`` alone uses the default tolerance of ``solve_iterate_vjp`` (1e-6 on f64,
        required on f32).  Without ``fixed`` and ``U`` nothing is clamped.  A mask on a 12/4 handle
        needs N <= 64 (``MpcbError``, MPCB_E_UNSUPPORTED); 17/6 has no such limit.

        ``model``: a vehicle per instance (mpcb_solve_gains_pm; 12/4 model), records [B|1, 14] as
        for ``solve_iterate``: the gains of that solve with the handle's weights."""
        torch = _torch()
        if not want_K and not want_P0:
            raise ValueError('solve_iterate_gains: want_K and want_P0 are both False')
        if self.nx == 17 and wind is not None:
            raise _lib.MpcbError('mpcb error -4: wind is a 12/4-model extension')
        if active_tol is not None and U is None and fixed is None:
            raise ValueError('active_tol needs U (the solve\'s output) to build the mask from')
        N = self.cfg.N
        xb, _ = self._dev(xbar, (N + 1, self.nx), 'xbar')
        B = xb.shape[0]
        if B > self.max_batch:
            raise ValueError(f'batch {B} > max_batch {self.max_batch}')
        ub, _ = self._dev(ubar, (N, self.nu), 'ubar', B)
        Ud = None if U is None else self._dev(U, (N, self.nu), 'U', B)[0]
        wd, wd_sb = (None, 0) if wind is None else self._dev(wind, (3,), 'wind', B, allow_broadcast=True)
        dev = self._tdev
        if fixed is not None:
            if isinstance(fixed, np.ndarray) and not fixed.flags.writeable:
                fixed = fixed.copy()   # torch.as_tensor warns on read-only arrays
            fx = torch.as_tensor(fixed, device=dev)
            if tuple(fx.shape) != (B, N, self.nu):
                raise ValueError(f'fixed: expected shape [{B}, {N}, {self.nu}], got {tuple(fx.shape)}')
            fx = (fx != 0).to(torch.uint8).contiguous()
        elif Ud is not None and (self.nx == 17 or active_tol is not None):
            fx = self.active_mask(Ud, active_tol)
        else:
            fx = None
        out = dict(K=torch.empty((B, N, self.nu, self.nx), dtype=self.dtype, device=dev) if want_K else None,
                   P0=torch.empty((B, self.nx, self.nx), dtype=self.dtype, device=dev) if want_P0 else None,
                   status=torch.empty((B,), dtype=torch.int32, device=dev), fixed=fx)
        if model is not None:
            md, m_sb = self._model_arg(model, B)
            self._keep_gains = (xb, ub, Ud, fx, wd, md)
            _lib.check(self.lib.mpcb_solve_gains_pm(
                self._h, B, self._ptr(xb), self._ptr(ub), self._ptr(Ud if fx is None else None), self._ptr(fx),
                self._ptr(wd), wd_sb, self._ptr(md), m_sb, self._ptr(out['K']), self._ptr(out['P0']),
                self._ptr(out['status']), self._stream()))
            return out
        self._keep_gains = (xb, ub, Ud, fx, wd)
        _lib.check(self.lib.mpcb_solve_gains(
            self._h, B, self._ptr(xb), self._ptr(ub), self._ptr(Ud if fx is None else None), self._ptr(fx),
            self._ptr(wd), wd_sb, self._ptr(out['K']), self._ptr(out['P0']), self._ptr(out['status']),
            self._stream()))
        return out

    def solve_iterate_diff(self, x0, xbar, ubar, x_ref, u_ref, wind=None, Q=None, R=None, QN=None,
                           active_tol=None, per_instance_weights=False, state_active_tol=None):
        """``solve_iterate`` as a differentiable torch operation: returns (u0, X, U) whose
        gradients flow to ``x0``, ``x_ref`` and ``u_ref`` and, when given, to the weight tensors
        ``Q``, ``R``, ``QN``, which the forward pass installs with ``set_weights`` (see
        ``mpc_blaster_amd.autograd``).  ``active_tol``: the 17/6 active-set tolerance of
        ``solve_iterate_vjp``.  ``per_instance_weights=True`` (12/4): the weight tensors follow the
        batch-axis rule of ``solve_iterate`` and go to the solve as arguments; the handle's weights
        stay as they are and nothing synchronises.  ``state_active_tol``: on a 17/6 state-box handle,
        the tolerance of the active state rows (``active_mask17x``); the backward pass is then the
        product with those rows (mpcb_solve_vjp17_sx), and an instance whose product reports a
        status other than 0 (a nearly dependent active set) gets zero gradients, like one whose
        forward status is not 0.  Without it such a handle is refused."""
        from .autograd import solve_iterate_diff
        return solve_iterate_diff(self, x0, xbar, ubar, x_ref, u_ref, wind, Q=Q, R=R, QN=QN,
                                  active_tol=active_tol, per_instance_weights=per_instance_weights,
                                  state_active_tol=state_active_tol)

    def solve_iterate_diff_pw17(self, x0, xbar, ubar, x_ref, u_ref, Q=None, R=None, QN=None, active_tol=None,
                                state_active_tol=None):
        """``solve_iterate_pw17`` as a differentiable torch operation: (u0, X, U) whose gradients flow
        to ``x0``, ``x_ref``, ``u_ref`` and the per-instance weight tensors, each in its own shape
        (``mpc_blaster_amd.autograd.solve_iterate_diff_pw17``).  The handle's weights stay as they
        are and nothing synchronises.  ``state_active_tol``: as in ``solve_iterate_diff``."""
        from .autograd import solve_iterate_diff_pw17
        return solve_iterate_diff_pw17(self, x0, xbar, ubar, x_ref, u_ref, Q=Q, R=R, QN=QN, active_tol=active_tol,
                                       state_active_tol=state_active_tol)

    def set_weights(self, Q=None, R=None, QN=None):
        """New cost weights on this handle (mpcb_set_weights; acados ``cost_set(k, 'W', W)`` with
        the same W on every stage, and ``W_e``): no re-creation of the handle or its workspace.
        Each of ``Q`` [12] or [12,12], ``R`` [4] or [4,4], ``QN`` like Q (17 / 6 on the full
        model) is a vector (the diagonal) or a symmetric matrix, NumPy or torch; None keeps the
        current one.  The values are read on the host, so a device tensor costs a
        synchronisation, and the call waits for the device: a configuration call like
        ``set_t_blast``.  Afterwards the handle solves like one created with the new weights."""
        mats = []
        for name, w, n in (('Q', Q, self.nx), ('R', R, self.nu), ('QN', QN, self.nx)):
            if w is None:
                mats.append(None)
                continue
            if hasattr(w, 'detach'):
                w = w.detach().cpu().numpy()
            w = np.asarray(w, dtype=np.float64)
            if w.shape == (n,):
                w = np.diag(w)
            if w.shape != (n, n):
                raise ValueError(f'{name}: expected [{n}] or [{n}, {n}], got {w.shape}')
            mats.append(np.ascontiguousarray(w))
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(self.lib.mpcb_set_weights(self._h, *[None if m is None else m.ctypes.data_as(dp) for m in mats]))
        for name, m in zip(('Q', 'R', 'QN'), mats):
            if m is not None:
                setattr(self.cfg, name, m.copy())
        self._c = self.cfg.to_c()
        self._weights_version += 1

    def set_params(self, p):
        """Parameters of the full 17/6 model (acados ``set(k, 'p', p)``,
        simulation_blaster.py:65-69): column-major J_angles 3x2, J_euler 3x3, J_p 3x3, T_blast.

        Shapes: [25] or [B|1, 25] (every stage alike), or [B|1, N|N+1, 25] stage by stage (the
        terminal stage N has no dynamics; its row is ignored).  ``None`` restores the defaults
        (zeros, T_blast = ``config.t_blast`` / ``set_t_blast``).

        An accepted call bumps ``_model_version``: the backward pass of a ``solve_iterate_diff``
        whose forward pass ran before it raises ``RuntimeError`` (``mpc_blaster_amd.autograd``)."""
        if self.nx != 17:
            raise ValueError('set_params is for the 17/6 model; the 12/4 slice takes set_t_blast')
        if p is None:
            _lib.check(self.lib.mpcb_set_params(self._h, 0, ctypes.c_void_p(0), 0, 0))
            self._params = None
            self._model_version += 1
            self._model_setter = 'set_params'
            return
        torch = _torch()
        N = self.cfg.N
        if isinstance(p, np.ndarray) and not p.flags.writeable:
            p = p.copy()   # torch.as_tensor warns on read-only arrays
        t = torch.as_tensor(p, dtype=self.dtype, device=self._tdev)
        if t.dim() == 1:
            t = t.reshape(1, 1, -1)
        elif t.dim() == 2:
            t = t.unsqueeze(1)
        if t.dim() != 3 or t.shape[-1] != 25 or t.shape[1] not in (1, N, N + 1):
            raise ValueError(f'p: expected [25], [B|1, 25] or [B|1, N|N+1, 25], got {tuple(p.shape)}')
        # acados ``set`` copies: a private device copy, so later writes to the caller's tensor
        # do not reach the solver (the library reads the pointer at every solve, mpcb.h)
        t = t.contiguous().clone()
        rows, stages = t.shape[0], t.shape[1]
        sb = 0 if rows == 1 else stages * 25
        kb = 0 if stages == 1 else 25
        _lib.check(self.lib.mpcb_set_params(self._h, rows, self._ptr(t), sb, kb))
        self._params = t   # the library keeps the device pointer: hold the tensor
        self._model_version += 1
        self._model_setter = 'set_params'

    def set_t_blast(self, t_blast: float):
        """Blaster thrust p[24] (blastermodel.py:210) as a scalar for every instance and stage:
        the 12/4 slice's body-z force; on the 17/6 model the default parameter vector's T_blast.
        Updates the handle in place (no re-creation).  Bumps ``_model_version``: the backward pass
        of a ``solve_iterate_diff``, or of a ``sim_step_diff`` without a ``model`` record, whose
        forward pass ran before it raises ``RuntimeError`` (``mpc_blaster_amd.autograd``)."""
        _lib.check(self.lib.mpcb_set_t_blast(self._h, float(t_blast)))
        self.cfg.t_blast = float(t_blast)
        self._model_version += 1
        self._model_setter = 'set_t_blast'

    def qp_stats(self, B=None):
        """Input-box work statistics of the last solve: int32 [B, 2] device tensor per instance
        (mpcb_qp_stats): 12/4 (forward passes, masked backward stages); 17/6 (interior-point
        iterations, polish passes)."""
        torch = _torch()
        B = self._u0.shape[0] if B is None else int(B)
        out = torch.empty((B, 2), dtype=torch.int32, device=self._tdev)
        _lib.check(self.lib.mpcb_qp_stats(self._h, B, self._ptr(out), self._stream()))
        return out

    def get_control(self):
        """First-step control u0* of the last solve, [B,4] device tensor."""
        if self._u0 is None:
            raise RuntimeError('solve() has not been called')
        return self._u0

    def get_state_trajectory(self):
        """Predicted state trajectory X = xbar + dx of the last solve, [B,N+1,12]."""
        if self._X is None:
            raise RuntimeError('no trajectory: call solve(..., want_traj=True)')
        return self._X

    def get_input_trajectory(self):
        if self._U is None:
            raise RuntimeError('no trajectory: call solve(..., want_traj=True)')
        return self._U

    def get_status(self):
        return self._status

    def linearize(self, xbar, ubar, wind=None):
        """A [B,N,12,12], B [B,N,12,4], Phi(xbar_k, ubar_k) [B,N,12] (debug / parity)."""
        torch = _torch()
        N = self.cfg.N
        xb, _ = self._dev(xbar, (N + 1, self.nx), 'xbar')
        B = xb.shape[0]
        ub, _ = self._dev(ubar, (N, self.nu), 'ubar', B)
        wd, wd_sb = (None, 0) if wind is None else self._dev(wind, (3,), 'wind', B, allow_broadcast=True)
        dev = self._tdev
        A = torch.empty((B, N, self.nx, self.nx), dtype=self.dtype, device=dev)
        Bm = torch.empty((B, N, self.nx, self.nu), dtype=self.dtype, device=dev)
        xn = torch.empty((B, N, self.nx), dtype=self.dtype, device=dev)
        _lib.check(self.lib.mpcb_linearize(self._h, B, self._ptr(xb), self._ptr(ub), self._ptr(wd),
                                           wd_sb, self._ptr(A), self._ptr(Bm), self._ptr(xn),
                                           self._stream()))
        self._keep = (xb, ub, wd)
        return A, Bm, xn

    def _params_arg(self, params, B):
        """A ``params=`` argument of the 17/6 plant step as (device tensor, stride): parameter vectors
        [25] or [B|1, 25] in the layout of ``set_params``; wider rows are padding that the library
        never reads."""
        torch = _torch()
        if self.nx != 17:
            raise ValueError('params covers the 17/6 model only (12/4: model)')
        if isinstance(params, np.ndarray) and not params.flags.writeable:
            params = params.copy()   # torch.as_tensor warns on read-only arrays
        t = torch.as_tensor(params, dtype=self.dtype, device=self._tdev)
        if t.dim() == 1:
            t = t.unsqueeze(0)
        if t.dim() != 2 or t.shape[1] < 25:
            raise ValueError(f'params: expected [25] or [B|1, 25] (or wider, padded rows), got {tuple(t.shape)}')
        if t.shape[0] != B and t.shape[0] != 1:
            raise ValueError(f'params: batch {t.shape[0]} != {B}')
        t = t.contiguous()
        return t, 0 if t.shape[0] == 1 else t.shape[1]

    def sim_step(self, x, u, T=None, wind=None, model=None, params=None):
        """Plant integrator: one RK4 step of length T (default dt) — AcadosSimSolver.solve().
        ``model``: a vehicle per instance (mpcb_sim_step_pm; 12/4 model), records [B|1, 14] as
        ``pack_model`` builds them; an instance with a non-finite record entry gets a NaN row.
        ``params``: the plant's parameter vectors (mpcb_sim_step_p17; 17/6 model), [25] or
        [B|1, 25] in the layout of ``set_params``, which stays the controller's belief; a 12/4 handle
        raises ``ValueError``."""
        torch = _torch()
        xs, _ = self._dev(x, (self.nx,), 'x')
        B = xs.shape[0]
        us, _ = self._dev(u, (self.nu,), 'u', B)
        wd, wd_sb = (None, 0) if wind is None else self._dev(wind, (3,), 'wind', B, allow_broadcast=True)
        xo = torch.empty_like(xs)
        if params is not None:
            pd, p_sb = self._params_arg(params, B)
            if wind is not None or model is not None:
                raise ValueError('wind and model are 12/4-model arguments: not together with params')
            _lib.check(self.lib.mpcb_sim_step_p17(self._h, B, self._ptr(xs), self._ptr(us), self._ptr(pd), p_sb,
                                                  float(self.cfg.dt if T is None else T), self._ptr(xo),
                                                  self._stream()))
            self._keep = (xs, us, pd)
            return xo
        if model is not None:
            md, m_sb = self._model_arg(model, B)
            _lib.check(self.lib.mpcb_sim_step_pm(self._h, B, self._ptr(xs), self._ptr(us), self._ptr(wd), wd_sb,
                                                 self._ptr(md), m_sb, float(self.cfg.dt if T is None else T),
                                                 self._ptr(xo), self._stream()))
            self._keep = (xs, us, wd, md)
            return xo
        _lib.check(self.lib.mpcb_sim_step(self._h, B, self._ptr(xs), self._ptr(us), self._ptr(wd),
                                          wd_sb, float(self.cfg.dt if T is None else T),
                                          self._ptr(xo), self._stream()))
        self._keep = (xs, us, wd)
        return xo

    def sim_step_vjp(self, x, u, gxn, T=None, wind=None, model=None, want=('gx', 'gu')):
        """Reverse mode of ``sim_step`` (mpcb_sim_step_vjp; 12/4 model): with ``gxn`` [B,12] the
        cotangent of the step's output, a dict of device tensors with the keys of ``want``, any
        non-empty subset of ``gx`` [B,12], ``gu`` [B,4], ``gwind`` [B,3], ``gmodel`` [B,14]
        (MPCB_MODEL_REC order; entry 0 is d/d mass, the nine entries of J independent).  ``T``,
        ``wind`` and ``model`` as for ``sim_step``; a broadcast ``wind`` / ``model`` still gives rows
        per instance, which the caller sums.  Without ``model``, ``gmodel`` is the gradient at the
        record of the handle's config.  An instance with a non-finite input gets NaN rows."""
        torch = _torch()
        if self.nx == 17:
            raise ValueError('sim_step_vjp covers the 12/4 model only')
        cols = dict(gx=self.nx, gu=self.nu, gwind=3, gmodel=_lib.MODEL_REC)
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or len(set(want)) != len(want) or set(want) - set(cols):
            raise ValueError(f'want: a non-empty subset of {tuple(cols)}, got {want}')
        xs, _ = self._dev(x, (self.nx,), 'x')
        B = xs.shape[0]
        if B > self.max_batch:
            raise ValueError(f'batch {B} > max_batch {self.max_batch}')
        us, _ = self._dev(u, (self.nu,), 'u', B)
        gn, _ = self._dev(gxn, (self.nx,), 'gxn', B)
        wd, wd_sb = (None, 0) if wind is None else self._dev(wind, (3,), 'wind', B, allow_broadcast=True)
        md, m_sb = (None, 0) if model is None else self._model_arg(model, B)
        out = {k: torch.empty((B, cols[k]), dtype=self.dtype, device=self._tdev) for k in want}
        _lib.check(self.lib.mpcb_sim_step_vjp(self._h, B, self._ptr(xs), self._ptr(us), self._ptr(wd), wd_sb,
                                              self._ptr(md), m_sb, float(self.cfg.dt if T is None else T),
                                              self._ptr(gn), *(self._ptr(out.get(k)) for k in cols),
                                              self._stream()))
        self._keep = (xs, us, gn, wd, md)
        return out

    def sim_step_vjp17(self, x, u, gxn, T=None, params=None, want=('gx', 'gu')):
        """Reverse mode of ``sim_step`` on the 17/6 model (mpcb_sim_step_vjp17): with ``gxn`` [B,17]
        the cotangent of the step's output, a dict of device tensors with the keys of ``want``, any
        non-empty subset of ``gx`` [B,17], ``gu`` [B,6], ``gparams`` [B,25] (the parameter vector's
        own order; entry 24 is d/d T_blast).  ``T`` and ``params`` as for ``sim_step``; a broadcast
        ``params`` still gives rows per instance, which the caller sums.  Without ``params``,
        ``gparams`` is the gradient at the handle's ``set_params`` rows (stage 0) or the defaults.
        An instance with a non-finite input gets NaN rows.  A 12/4 handle raises ``ValueError``."""
        torch = _torch()
        if self.nx != 17:
            raise ValueError('sim_step_vjp17 covers the 17/6 model only (12/4: sim_step_vjp)')
        cols = dict(gx=self.nx, gu=self.nu, gparams=25)
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or len(set(want)) != len(want) or set(want) - set(cols):
            raise ValueError(f'want: a non-empty subset of {tuple(cols)}, got {want}')
        xs, _ = self._dev(x, (self.nx,), 'x')
        B = xs.shape[0]
        if B > self.max_batch:
            raise ValueError(f'batch {B} > max_batch {self.max_batch}')
        us, _ = self._dev(u, (self.nu,), 'u', B)
        gn, _ = self._dev(gxn, (self.nx,), 'gxn', B)
        pd, p_sb = (None, 0) if params is None else self._params_arg(params, B)
        out = {k: torch.empty((B, cols[k]), dtype=self.dtype, device=self._tdev) for k in want}
        _lib.check(self.lib.mpcb_sim_step_vjp17(self._h, B, self._ptr(xs), self._ptr(us), self._ptr(pd), p_sb,
                                                float(self.cfg.dt if T is None else T), self._ptr(gn),
                                                *(self._ptr(out.get(k)) for k in cols), self._stream()))
        self._keep = (xs, us, gn, pd)
        return out

    def sim_step_diff17(self, x, u, T=None, params=None):
        """``sim_step`` on the 17/6 model as a differentiable torch operation: gradients flow to the
        tensors ``x``, ``u`` and ``params`` (see ``mpc_blaster_amd.autograd.sim_step_diff17``)."""
        from .autograd import sim_step_diff17
        return sim_step_diff17(self, x, u, T=T, params=params)

    def sim_step_diff(self, x, u, T=None, wind=None, model=None):
        """``sim_step`` as a differentiable torch operation: gradients flow to the tensors ``x``,
        ``u``, ``wind`` and ``model`` (see ``mpc_blaster_amd.autograd.sim_step_diff``)."""
        from .autograd import sim_step_diff
        return sim_step_diff(self, x, u, T=T, wind=wind, model=model)

    def gen_inputs(self, B, seed, id_offset=0, ref='hover', wind=False):
        """Synthetic inputs on device (SURVEY §8 d): x0 [B,12], x_ref, u_ref (broadcast for hover)."""
        torch = _torch()
        N = self.cfg.N
        dev = self._tdev
        x0 = torch.empty((B, self.nx), dtype=self.dtype, device=dev)
        if ref == 'sine':
            xr = torch.empty((B, N + 1, self.nx), dtype=self.dtype, device=dev)
            xr_sb, kind = (N + 1) * self.nx, 1
        else:
            xr = torch.empty((1, N + 1, self.nx), dtype=self.dtype, device=dev)
            xr_sb, kind = 0, 0
        ur = torch.empty((1, N, self.nu), dtype=self.dtype, device=dev)
        wd = torch.empty((B, 3), dtype=self.dtype, device=dev) if wind else None
        _lib.check(self.lib.mpcb_gen_inputs(self._h, B, int(seed), int(id_offset), kind,
                                            self._ptr(x0), self._ptr(xr), xr_sb, self._ptr(ur), 0,
                                            self._ptr(wd), self._stream()))
        return dict(x0=x0, xref=xr, uref=ur, wind=wd)

    def histogram(self, u0, lo=0.0, hi=65.0, nbins=64, counts=None):
        """Accumulate a per-motor histogram of u0 into int64 counts [4, nbins] (device)."""
        torch = _torch()
        u, _ = self._dev(u0, (self.nu,), 'u0')
        if counts is None:
            counts = torch.zeros((self.nu, nbins), dtype=torch.int64, device=self._tdev)
        _lib.check(self.lib.mpcb_histogram(self._h, u.shape[0], self._ptr(u), float(lo), float(hi),
                                           int(nbins), self._ptr(counts), self._stream()))
        return counts
