/*
 * mpcb.h — C ABI of libmpcblaster.so, the MI355X-native batched MPC hot path.
 *
 * Drop-in boundary for the per-control-step solve of sml93/mpc_blaster.  The reference crosses
 * this boundary once per control step at ``ocp_solver.solve()``
 * (src/scripts/simulation_blaster.py:80, mavros_blaster_sim.py:85), i.e. acados'
 * AcadosOcpSolver over its ctypes-loaded generated library; the plant step is
 * ``integrator.solve()`` (simulation_blaster.py:94-104, AcadosSimSolver).  Each entry point
 * below names the reference interface it replaces.
 *
 * Conventions
 *  - Plain C: pointers + sizes, no C++ or torch types.  Every call returns 0 or a negative
 *    MPCB_E_* code; ``mpcb_last_error()`` gives a thread-local message.
 *  - Array arguments are DEVICE pointers (HBM, caller-owned, e.g. torch ROCm tensors) of the
 *    handle's dtype (double when cfg.dtype == MPCB_F64, float when MPCB_F32).  Per-instance
 *    strides are in ELEMENTS; a stride of 0 broadcasts one array to the whole batch.  A stride
 *    may exceed the record's length (padded records); a negative stride is refused with
 *    MPCB_E_INVALID by every entry point that takes one.
 *  - Alignment: input arrays, u0, status and every other output need only the alignment of their
 *    element type (8 bytes for double, 4 for float and int32), at the base and at every record;
 *    the solves' X and U outputs alone must be 16-byte aligned.  A call writes nothing outside
 *    the arrays it is given.
 *  - Calls are asynchronous on ``hip_stream`` (NULL = default stream).  The Python facade
 *    synchronises to keep acados' synchronous semantics.
 *  - A handle is bound to one device, owns its workspace, and is not re-entrant.
 *  - Per-instance ``status`` (acados codes: 0 success, 1 NaN detected, 2 max iterations,
 *    3 MINSTEP, 4 QP failure) is separate from the call-level return code.
 *  - Arrays handed to a setter (mpcb_set_params) are read by later solves, not copied: the
 *    caller keeps them alive and unchanged until the next set call (the Python facade passes a
 *    private copy, so it keeps acados' copy semantics of ``set``).
 */
#ifndef MPCB_H
#define MPCB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPCB_ABI_VERSION 5

enum { MPCB_F64 = 0, MPCB_F32 = 1 };
enum { MPCB_MODE_ROLLOUT = 0, MPCB_MODE_ITERATE = 1 };
enum {
  MPCB_OK = 0,
  MPCB_E_INVALID = -1,   /* bad argument / shape */
  MPCB_E_HIP = -2,       /* HIP runtime error */
  MPCB_E_NOMEM = -3,     /* workspace allocation failed */
  MPCB_E_UNSUPPORTED = -4
};
/* per-instance solver status, acados' codes (ACADOS_SUCCESS, _NAN_DETECTED, _MAXITER, _MINSTEP,
 * _QP_FAILURE).  MINSTEP: the fp64 17/6 interior point stopped at its conditioning limit (a
 * breakdown or collapsed step once mu <= 1e-5 on a feasible iterate) and no active-set polish
 * certified the point: the outputs are that reduced-accuracy iterate.  With the state box the
 * polish runs first (MINSTEP = it did not certify); the input box alone (Mehrotra) has no polish,
 * so every such stop there reports MINSTEP (oracle: ocp._ipm_box_mehrotra, the same rule). */
enum { MPCB_STATUS_OK = 0, MPCB_STATUS_NAN = 1, MPCB_STATUS_MAXITER = 2, MPCB_STATUS_MINSTEP = 3,
       MPCB_STATUS_QP_FAIL = 4 };

#define MPCB_MAX_NX 17
#define MPCB_MAX_NU 6

/*
 * A vehicle per instance (12/4 model): the model record.  One instance's vehicle is MPCB_MODEL_REC
 * elements of the handle's dtype in a DEVICE array:
 *   [0] mass  [1] lx  [2] ly  [3] c  [4] t_blast  [5..13] J, row-major 3x3
 * Gravity, dt and the boxes stay with the handle.  The entry points that take a record
 * (mpcb_sim_step_pm, mpcb_solve_iterate_pm, mpcb_solve_gains_pm, mpcb_sim_step_vjp) take it as
 * `model, model_sb`:
 *   instance b's record starts at model + b * model_sb, in elements;
 *   model_sb == 0 broadcasts one record; model_sb >= MPCB_MODEL_REC is allowed and the pad elements
 *   are never read; 0 < model_sb < MPCB_MODEL_REC or a negative stride is MPCB_E_INVALID;
 *   the array needs element alignment only;
 *   model == NULL means the handle's own model, and the call then launches the kernels of its
 *   counterpart without `_pm` and returns its bits.
 * The device derives 1 / mass and the inverse of J: the inverse by the adjugate formula in fp64
 * from the record's values, rounded to the handle's dtype, so a record equal to the handle's config
 * gives the handle's own model up to the rounding of the division order.  The library cannot
 * validate device data: mass > 0 and a symmetric positive definite (so invertible) J are the
 * caller's contract.  Every record entry joins the NaN rule of the call it is given to.
 * Out of scope, each refused or absent: the 17/6 model (its per-instance data are mpcb_set_params);
 * rollout mode (mpcb_solve); the tuned shared-weight solve paths (mpcb_solve_iterate and the bench
 * configs c1-c5 keep one vehicle per handle); mpcb_eval, mpcb_linearize, the mpcb_solve_vjp family
 * and the torch layer at per-instance models; gradients of the RTI step with respect to the model
 * (the plant step offers the model gradient: mpcb_sim_step_vjp); fp32 with the input box;
 * per-instance gravity, dt or boxes.
 */
#define MPCB_MODEL_REC 14

/*
 * Problem definition: replaces the ``blasterModel(mass, J, l_x, l_y, N, Tf, c, Q, R, Q_t,
 * blastThruster, statesBound, controlBound)`` constructor + ``generateController()``
 * (src/scripts/blastermodel.py:16, :214-292) that build the acados OCP.
 * Matrices are row-major, leading dimension nx (Q, QN) or nu (R).
 * Q, R and QN must be symmetric: the kernels read them transposed in some tables and straight in
 * others, so a config in which one of them differs from its transpose by more than
 * 1e-12 * max|entry| is refused with MPCB_E_INVALID (by mpcb_create, mpcb_plan_kernels and
 * mpcb_debug_row_table alike).  Dense symmetric weights are supported on every path.
 */
typedef struct mpcb_config {
  int32_t nx;            /* 12 (rigid-body slice, the BASELINE configs) or 17 (full model) */
  int32_t nu;            /* 4 or 6 */
  int32_t N;             /* horizon (ocp.dims.N, blastermodel.py:226) */
  int32_t dtype;         /* MPCB_F64 | MPCB_F32 */
  int32_t box_u;         /* 1: lbu <= u <= ubu on stages 0..N-1 (idxbu, blastermodel.py:261) */
  int32_t max_as_iter;   /* box_u iteration cap.  17/6: interior-point iterations.  12/4: active-set
                            passes, at most 48 (AS_IPM_AFTER); an instance not converged by then is
                            solved by the interior point (<= 100 iterations, mpcb_asipm.h) */
  int32_t box_x;         /* 17/6 only, needs box_u: lbx <= x_k <= ubx on stages 1..N-1 (idxbx,
                            blastermodel.py:268-270 statesBound; JSON constraints.lbx/ubx) */
  int32_t reserved;
  double dt;             /* Tf / N (solver_options.tf, blastermodel.py:287) */
  double cost_scale;     /* stage-cost scaling; acados uses time_steps[k] = dt */
  double mass, lx, ly, c, g, t_blast;   /* 17/6: t_blast is the default parameter p[24] */
  double J[9];           /* inertia (row-major 3x3) */
  double Q[MPCB_MAX_NX * MPCB_MAX_NX];   /* stage state weight  (W[:nx,:nx]) */
  double R[MPCB_MAX_NU * MPCB_MAX_NU];   /* stage input weight  (W[nx:,nx:]) */
  double QN[MPCB_MAX_NX * MPCB_MAX_NX];  /* terminal weight (W_e = Q_t) */
  double lbu[MPCB_MAX_NU], ubu[MPCB_MAX_NU];
  double lbx[MPCB_MAX_NX], ubx[MPCB_MAX_NX];   /* state box (box_x) */
} mpcb_config;

typedef struct mpcb_handle mpcb_handle;

/* Library / device lifetime.  Replaces AcadosOcpSolver(ocp, json_file) construction
 * (blastermodel.py:289): validates the config, uploads weights, sizes the workspace. */
int mpcb_create(const mpcb_config* cfg, int device, int64_t max_batch, mpcb_handle** out);
int mpcb_destroy(mpcb_handle* h);
const char* mpcb_last_error(void);
int mpcb_abi_version(void);
/* Workspace bytes owned by the handle (informational). */
int64_t mpcb_workspace_bytes(const mpcb_handle* h);
/* Kernel path chosen at creation: 1 = split nominal / Riccati / forward kernels (unconstrained),
 * 0 = single-kernel solver (input boxes; small batches when MPCB_SPLIT_MIN_BATCH asks for it). */
int mpcb_path(const mpcb_handle* h);
/* Optional device timing of later solves: HIP events recorded on the launch stream around each
 * kernel phase.  ``mpcb_last_timing`` waits for the last timed solve and writes the device
 * milliseconds of its phases: ms[0] nominal rollout, ms[1] Riccati (the dominant kernel; the
 * single launch on the fused / box paths), ms[2] forward pass; on the 17/6 model ms[0] nominal17,
 * ms[1] riccati17 (Riccati + forward, the interior point with boxes), ms[2] lin17ws (the
 * stage-parallel linearisation).  Summed over chunks (up to 64).
 * No reference counterpart (acados' ``get_stats('time_tot')`` is host wall time). */
int mpcb_set_timing(mpcb_handle* h, int enable);
int mpcb_last_timing(mpcb_handle* h, float ms[3]);
/* Kernels of a solve, one line per timing phase (the slots of mpcb_last_timing: nominal, Riccati,
 * forward pass / 17/6 linearisation; a fourth line for the small-chunk path's linearisation),
 * as rocprofv3 names the dispatches ("mpcb::riccati_kernel_f32<false, false, false>"), an empty
 * line for a phase without a launch; NUL-terminated in buf[len].
 * mpcb_plan_kernels: what mpcb_solve (mode MPCB_MODE_ROLLOUT, want_traj: X and U requested) or
 * mpcb_solve_iterate (MPCB_MODE_ITERATE) of B instances would launch on a handle created with
 * (cfg, max_batch) -- the same selection code, run without a device (no HIP call).
 * mpcb_last_kernels: what the handle's last solve launched.
 * No reference counterpart (profiling aid: ties a roofline to the rocprof dispatch it cites). */
int mpcb_plan_kernels(const mpcb_config* cfg, int64_t max_batch, int64_t B, int mode, int want_traj,
                      char* buf, int64_t len);
int mpcb_last_kernels(const mpcb_handle* h, char* buf, int64_t len);

/*
 * One SQP_RTI step for B independent instances, linearised at the RK4 rollout of u_ref from
 * x0 (north_star surface ``solve(x0, x_ref, u_ref)``).  Replaces, per instance, the call
 * sequence ocp_solver.set(0,'lbx'/'ubx',x0) / cost_set(k,'yref',...) / solve() /
 * get(0,'u') / get(k,'x') (simulation_blaster.py:60-89).
 *   x0    [B, nx]            stride x0_sb
 *   xref  [B|1, N+1, nx]     stride xref_sb (0 = broadcast)
 *   uref  [B|1, N, nu]       stride uref_sb
 *   wind  [B|1, 3] or NULL   world-frame disturbance force (build extension, c5)
 *   u0    [B, nu]            first-step control u0* (required)
 *   X     [B, N+1, nx]|NULL  predicted state trajectory xbar + dx (linear prediction)
 *   U     [B, N, nu]|NULL    predicted controls (X and U 16-byte aligned)
 *   status[B] int32          per-instance status
 */
int mpcb_solve(mpcb_handle* h, int64_t B,
               const void* x0, int64_t x0_sb,
               const void* xref, int64_t xref_sb,
               const void* uref, int64_t uref_sb,
               const void* wind, int64_t wind_sb,
               void* u0, void* X, void* U, int32_t* status, void* hip_stream);

/*
 * acados SQP_RTI semantics: linearise at the persistent iterate (xbar [B,N+1,nx],
 * ubar [B,N,nu]) with gaps, x0 enforced through dx_0 = x0 - xbar_0; outputs the full-step
 * iterate X = xbar + dx, U = ubar + du (X/U may alias xbar/ubar).  This is what one
 * ``ocp_solver.solve()`` does on the persistent solver object (simulation_blaster.py:80).
 */
int mpcb_solve_iterate(mpcb_handle* h, int64_t B,
                       const void* x0, int64_t x0_sb,
                       const void* xbar, const void* ubar,
                       const void* xref, int64_t xref_sb,
                       const void* uref, int64_t uref_sb,
                       const void* wind, int64_t wind_sb,
                       void* u0, void* X, void* U, int32_t* status, void* hip_stream);

/*
 * Linearisation only (debug / parity): RK4 + exact forward sensitivities of every shooting
 * interval.  A [B,N,nx,nx], Bm [B,N,nx,nu], xnext [B,N,nx] = Phi(xbar_k, ubar_k).
 * Replaces acados sim_erk with sens_forward (what SQP_RTI evaluates inside solve()).
 */
int mpcb_linearize(mpcb_handle* h, int64_t B, const void* xbar, const void* ubar,
                   const void* wind, int64_t wind_sb,
                   void* A, void* Bm, void* xnext, void* hip_stream);

/*
 * Quality of a given iterate (X [B,N+1,nx], U [B,N,nu], contiguous; e.g. what a solve returned):
 * the objective and the KKT residuals per instance.  Replaces ``ocp_solver.get_cost()``
 * (simulation_blaster.py:86, mavros_blaster_sim.py:87) and acados' ``get_residuals()``.  Reads the
 * handle's weights, boxes, model, wind and 17/6 parameters as mpcb_solve_iterate does; s =
 * cfg.cost_scale.  Outputs are [B] arrays of the handle's dtype; any may be NULL, not all four.
 *   cost      1/2 s sum_{k<N} (|x_k - xref_k|^2_Q + |u_k - uref_k|^2_R) + 1/2 |x_N - xref_N|^2_QN
 *   res_eq    max_k |Phi(x_k, u_k) - x_{k+1}|_inf (the handle's RK4 step); with x0 [B,nx] given
 *             (may be NULL) also |x_0 - x0|_inf
 *   res_ineq  the largest violation of lbu <= u_k <= ubu (k < N, box_u) and of lbx <= x_k <= ubx
 *             (0 < k < N, box_x); never negative, 0 without boxes
 *   res_stat  the natural residual of the reduced gradient: lambda_N = QN (x_N - xref_N), and for
 *             k = N-1 .. 0, with A_k, B_k the exact RK4 sensitivities at (x_k, u_k),
 *               g_k = s R (u_k - uref_k) + B_k^T lambda_{k+1},
 *               lambda_k = s Q (x_k - xref_k) + A_k^T lambda_{k+1};
 *             res_stat = max_k |g_k|_inf, with box_u max_k |u_k - clip(u_k - g_k, lbu, ubu)|_inf.
 *             It is the gradient of the single-shooting objective when res_eq = 0, and merges
 *             stationarity with the input box's complementarity (no tolerance).  With box_x a
 *             non-NULL res_stat is MPCB_E_UNSUPPORTED: the state multipliers are not available.
 * An instance with a non-finite input gets NaN in every output; other instances are unaffected.
 */
int mpcb_eval(mpcb_handle* h, int64_t B,
              const void* x0, int64_t x0_sb,
              const void* X, const void* U,
              const void* xref, int64_t xref_sb,
              const void* uref, int64_t uref_sb,
              const void* wind, int64_t wind_sb,
              void* cost, void* res_eq, void* res_ineq, void* res_stat,
              void* hip_stream);

/*
 * Vector-Jacobian product of one mpcb_solve_iterate step (12/4 model, both dtypes, with and
 * without the input box).  Let J be the Jacobian of (X, U) with respect to (x0, xref, uref), taken
 * at fixed xbar, ubar, wind, weights, model and active set; the outputs are J^T (gX, gU):
 *   xbar [B,N+1,nx], ubar [B,N,nu]   the linearisation point the solve was given (xbar_N is not read)
 *   U    [B,N,nu]                    the solve's output, read only for the active set; NULL allowed
 *                                    iff the handle has no input box
 *   gX [B,N+1,nx], gU [B,N,nu]       cotangents of X and U; either may be NULL (= 0), not both.  A
 *                                    cotangent of u0 is added to gU[:, 0] by the caller
 *   gx0 [B,nx], gxref [B,N+1,nx], guref [B,N,nu]   the gradients; any may be NULL, not all.  For a
 *                                    broadcast reference (stride 0 in the solve) the caller sums over B
 * All arrays are contiguous.  In iterate mode the linearisation point does not depend on the
 * differentiated inputs, so (X, U) is affine in them on each active set and the product is exact:
 * one more LQ solve over the same [A_k | B_k] with linear terms (-gX, -gU), no gaps and dx_0 = 0.
 * xbar and ubar are treated as constants (Gauss-Newton / RTI): no gradient with respect to them,
 * the model or wind is offered (the cost weights: mpcb_solve_vjp_w below).  Rollout mode is not
 * covered: there the linearisation point depends on x0.
 * Active set: component (k, m) is clamped iff U[k,m] <= lbu[m] or U[k,m] >= ubu[m], compared in
 * the handle's dtype (the box kernels write the bound value itself into clamped components, so a
 * solve's own U gives its final set).  Clamped components have zero sensitivity.  At a degenerate
 * point (clamped with a zero multiplier) this is one of the valid one-sided derivatives.  An
 * instance that the active set handed to the interior point (mpcb_config.max_as_iter) returns U
 * inside the box, within that method's tolerance of the bounds and not on them: its clamped
 * components are not recognised and its product is the unconstrained one.
 * status[B]: MPCB_STATUS_OK; MPCB_STATUS_NAN for an instance with a non-finite input or cotangent
 * (its outputs are all NaN, other instances are unaffected); MPCB_STATUS_QP_FAIL when the masked
 * input Hessian of a stage is not positive definite.
 * MPCB_E_UNSUPPORTED on a 17/6 handle.  The workspace of this call is allocated by the first call
 * on the handle and is not part of what the handle's workspace size reports.
 * No reference counterpart (acados offers solution sensitivities through a separate solver build).
 */
int mpcb_solve_vjp(mpcb_handle* h, int64_t B,
                   const void* xbar, const void* ubar,
                   const void* U,
                   const void* wind, int64_t wind_sb,
                   const void* gX, const void* gU,
                   void* gx0, void* gxref, void* guref,
                   int32_t* status, void* hip_stream);

/*
 * mpcb_solve_vjp plus the gradients with respect to the cost weights, in the same launch.  With
 * L = <gX, X> + <gU, U> and (dx, du) the adjoint step of mpcb_solve_vjp (the solution that gives
 * gxref_k = s Q dx_k; du = 0 on clamped components, dx_0 = 0), at a fixed linearisation point and
 * active set
 *   rx_k = X_k - xref_k,  ru_k = U_k - uref_k      (X, U: what mpcb_solve_iterate returned)
 *   gQ  = -s sym(sum_{k<N} dx_k rx_k^T)   [B,nx,nx]
 *   gR  = -s sym(sum_{k<N} du_k ru_k^T)   [B,nu,nu]
 *   gQN =   -sym(dx_N rx_N^T)             [B,nx,nx]     sym(M) = (M + M^T) / 2,  s = cfg.cost_scale
 * row-major, of the handle's dtype, per instance (the weights are shared by the batch: the caller
 * sums over B; the kernel uses no atomics, so results are bit-reproducible) and bitwise symmetric.
 * Convention: the weights are symmetric matrices, so for any symmetric perturbation dQ of Q the
 * change of L is <gQ, dQ>_F (likewise R, QN); the derivative with respect to a diagonal entry is
 * gQ[i][i], with respect to the pair of entries (i, j) and (j, i) moved together 2 gQ[i][j].
 * Exact on the active set, like the product itself (L is not affine in the weights).
 *   X [B,N+1,nx], U [B,N,nu], xref / uref with the solve's strides (0 = broadcast): required iff
 *   one of gQ, gR, gQN is given; otherwise the rules of mpcb_solve_vjp hold (X, xref and uref are
 *   not read, U is required on an input-box handle only)
 *   any of the six outputs may be NULL, not all
 * A call without a weight output launches the kernels of mpcb_solve_vjp and returns its bits.
 * Inherited limit: an instance that the active set handed to the interior point has U inside the
 * box, so its clamped components are not recognised and its gradients are the unconstrained ones.
 * X, U, xref and uref join the NaN rule: a non-finite entry gives that instance status
 * MPCB_STATUS_NAN and NaN in all six outputs.  MPCB_E_UNSUPPORTED on a 17/6 handle, MPCB_E_INVALID
 * for a missing argument.
 */
int mpcb_solve_vjp_w(mpcb_handle* h, int64_t B,
                     const void* xbar, const void* ubar,
                     const void* X, const void* U,
                     const void* xref, int64_t xref_sb,
                     const void* uref, int64_t uref_sb,
                     const void* wind, int64_t wind_sb,
                     const void* gX, const void* gU,
                     void* gx0, void* gxref, void* guref,
                     void* gQ, void* gR, void* gQN,
                     int32_t* status, void* hip_stream);

/*
 * The product and the weight gradients of mpcb_solve_vjp / mpcb_solve_vjp_w for the full 17/6 model
 * (nx = 17, nu = 6; both dtypes).  The adjoint problem (linear terms (-gX, -gU), no gaps, dx_0 = 0),
 * the outputs gx0, gxref_k = s Q dx_k, gxref_N = QN dx_N, guref_k = s R du_k, the weight formulas
 * and their symmetry convention, per-instance results without atomics (bitwise symmetric gQ, gR,
 * gQN), the NaN rule, MPCB_STATUS_QP_FAIL for a masked input Hessian that is not positive definite
 * and the first-call allocation of the call's own workspace are those of the two 12/4 entry points
 * above, word for word.  What differs:
 *   fixed [B,N,6] uint8   the active set, given by the caller: nonzero = component (k, m) is clamped;
 *                         NULL = nothing is clamped.  The 17/6 boxes are solved by an interior
 *                         point, so U lies near its bounds and not on them, and no rule on U's bits
 *                         recovers the set: the caller derives it (a tolerance on U - lbu and
 *                         ubu - U; BatchedMPC.solve_iterate_vjp does that).  The product is exact
 *                         for the mask it is given, on any accepted handle whatever its box_u.  A
 *                         clamped component has du = 0 and a zero row of K (the stage's input
 *                         system with its row and column zeroed, the diagonal set to 1, and its
 *                         rows of H_ux and h_u zeroed); its guref entry is row m of s R du, which
 *                         is 0 for a diagonal R.  A stage with all six components clamped is valid.
 *   X, U, xref, uref      read only when a weight output is requested (then required, and part of
 *                         the NaN rule); U plays no part in the active set
 *   parameters            the handle's mpcb_set_params array with its strides, or the defaults:
 *                         what mpcb_solve_iterate reads.  B beyond the array's instance rows is
 *                         MPCB_E_INVALID unless it is broadcast.  A non-finite parameter joins the
 *                         NaN rule.  They are constants of the product: no gradient is offered.
 *   any of the six outputs may be NULL, not all; gx0, gxref and guref have the same bits with and
 *   without weight outputs
 * MPCB_E_UNSUPPORTED on a 12/4 handle, and on a handle with box_x: an active state row is a state
 * equality of the adjoint problem, which this call does not solve; mpcb_solve_vjp17_sx below does,
 * and with fixed_x == NULL it is this call for a caller who has checked that no state row is
 * active.  MPCB_E_INVALID:
 * no cotangent, no output, B > max_batch, a weight output without X, U, xref or uref, a negative
 * stride.  Large batches run in the chunks of the handle's solves; the workspace holds one chunk,
 * is allocated by the first call (MPCB_E_NOMEM) and is not counted by mpcb_workspace_bytes.
 */
int mpcb_solve_vjp17(mpcb_handle* h, int64_t B,
                     const void* xbar, const void* ubar,
                     const uint8_t* fixed,
                     const void* X, const void* U,
                     const void* xref, int64_t xref_sb,
                     const void* uref, int64_t uref_sb,
                     const void* gX, const void* gU,
                     void* gx0, void* gxref, void* guref,
                     void* gQ, void* gR, void* gQN,
                     int32_t* status, void* hip_stream);

/*
 * The local feedback law and the cost-to-go Hessian of the SQP_RTI step, on both models and in
 * both dtypes.  The call works on the LQ problem that mpcb_solve_iterate solves at (xbar, ubar),
 * with the handle's weights, model, wind (12/4) or parameters (17/6) and s = cfg.cost_scale:
 *   P_N = QN;  for k = N-1 .. 0, [A_k | B_k] the exact RK4 sensitivities at (xbar_k, ubar_k):
 *     H   = blkdiag(s Q, s R) + [A|B]^T P_{k+1} [A|B]
 *     H~  = H with the clamped input components masked: their rows and columns of H_uu zeroed and
 *           its diagonal set to 1 there, their rows of H_ux zeroed
 *     K_k = -H~uu^-1 H~ux                    (a clamped component's row is exactly 0, bitwise)
 *     P_k = H_xx + H_ux^T K_k                (the unmasked H_ux)
 * No gap, reference or linear term enters: neither K nor P depends on them.
 *   K  [B,N,nu,nx]   row-major, of the handle's dtype (acados: get_from_qp_in(k, 'K'))
 *   P0 [B,nx,nx]     P_0, bitwise symmetric             (acados: get_from_qp_in(0, 'P'))
 *   either may be NULL, not both; all arrays are contiguous; K and P0 need only element alignment;
 *   nothing outside K, P0 and status is written
 * What they mean.  On a fixed active set, in iterate mode, two solves that differ only in x0
 * return (X, U) and (X', U') with
 *   U'_k - U_k = K_k (X'_k - X_k)   for every k,   in particular  d u0 / d x0 = K_0,
 * which is the feedback u = U_j + K_j (x_meas - X_j) an RTI deployment applies between solves, and
 * the optimal value V of the solve's QP as a function of x0 satisfies
 *   V(x0 + d) + V(x0 - d) - 2 V(x0) = d^T P_0 d:   P_0 is the Hessian of the value function.
 * The active set:
 *   fixed [B,N,nu] uint8   nonzero = component (k, m) is clamped; accepted on both models, and the
 *                          result is exact for the mask it is given.  A stage with every component
 *                          clamped is valid (K_k = 0, P_k = H_xx).  On the 12/4 model the kernel
 *                          keeps one mask word per input, so `fixed` needs N <= 64 (the limit
 *                          mpcb_create sets for box_u there): MPCB_E_UNSUPPORTED beyond it.  The
 *                          17/6 model has no such limit.
 *   fixed == NULL          12/4 handle with the input box: U [B,N,nu] is required and the set is
 *                          read from it by the rule of mpcb_solve_vjp (on or beyond a bound);
 *                          12/4 handle without the box, or a 17/6 handle: nothing is clamped and U
 *                          is not read (the 17/6 caller derives `fixed`, see mpcb_solve_vjp17)
 * status[B]: MPCB_STATUS_OK; MPCB_STATUS_NAN for an instance with a non-finite xbar, ubar, wind,
 * parameter, or U where U is read (its outputs are all NaN, other instances keep their bits);
 * MPCB_STATUS_QP_FAIL when a masked input Hessian is not positive definite.
 * MPCB_E_UNSUPPORTED on a 17/6 handle with box_x (the reason given at mpcb_solve_vjp17), for
 * wind on a 17/6 handle and for fixed on a 12/4 handle with N > 64.  MPCB_E_INVALID: both outputs NULL, B > max_batch, a negative stride, a
 * 12/4 input-box handle with neither U nor fixed.  The workspace is allocated by the first call
 * (MPCB_E_NOMEM) and is not counted by mpcb_workspace_bytes; on the 17/6 model it is
 * mpcb_solve_vjp17's, and large batches run in the chunks of the handle's solves.
 */
int mpcb_solve_gains(mpcb_handle* h, int64_t B,
                     const void* xbar, const void* ubar,
                     const void* U, const uint8_t* fixed,
                     const void* wind, int64_t wind_sb,
                     void* K, void* P0, int32_t* status, void* hip_stream);

/*
 * mpcb_solve_iterate with the cost weights given per instance (12/4 model): the QP of
 * mpcb_solve_iterate at (xbar, ubar) in which instance b's own Q, R and QN stand in place of the
 * handle's (the stage cost stays s Q_b, s R_b with s = cfg.cost_scale; the terminal cost is QN_b).
 * The model, wind, dt, cost_scale and the input box come from the handle.  For a cost predicted
 * per sample by a network, or B candidate weightings in one batch.
 *   Qw [B|1,nx,nx], Rw [B|1,nu,nu], QNw [B|1,nx,nx]   DEVICE arrays of the handle's dtype, row-major;
 *        instance b's matrix starts at Qw + b * Qw_sb (elements; likewise Rw_sb, QNw_sb).  Stride 0
 *        broadcasts one matrix, a stride may exceed the record length, a negative stride is
 *        MPCB_E_INVALID.  A NULL pointer means the handle's own matrix.  The arrays need only
 *        element alignment.  Each matrix must be symmetric (and Q, QN positive semidefinite, R
 *        positive definite, as for mpcb_config): the library cannot check device data, and the
 *        kernel reads row j as column j.
 *   every other argument, the aliasing of X / U with xbar / ubar and the alignment rules are those
 *   of mpcb_solve_iterate
 * status[B]: MPCB_STATUS_OK; MPCB_STATUS_NAN for an instance with a non-finite entry anywhere in
 * its inputs, the weights included (its u0, X and U are all NaN; the other instances keep their
 * bits); MPCB_STATUS_QP_FAIL when a masked input Hessian H_uu is not positive definite;
 * MPCB_STATUS_MAXITER as below.
 * The input box (fp64 handles only) is solved by the primal-dual active set alone: full exchange of
 * the infeasible set V with the Kim-Park safeguard (3 tries) and the least-index backup rule, at
 * most min(cfg.max_as_iter, 48) passes, with no hand-over to the interior point, neither after the
 * first pass nor at the cap.  An instance that has not converged by then gets MPCB_STATUS_MAXITER
 * and the last pass's iterate.  A clamped component of U (and of u0) is the bound's value itself, so
 * the rule of mpcb_solve_vjp recovers the final set from U.  mpcb_qp_stats is not updated by this
 * call, and mpcb_last_kernels / mpcb_last_timing do not see it.
 * One self-contained kernel (16 lanes per instance); the handle's tuned solve paths are not used,
 * so with all three pointers NULL the result agrees with mpcb_solve_iterate to rounding, not bit
 * for bit.  The workspace is allocated by the first call (MPCB_E_NOMEM) and is not counted by
 * mpcb_workspace_bytes.
 * MPCB_E_UNSUPPORTED: a 17/6 handle; an fp32 handle with box_u (the shared-weight fp32 box owes its
 * accuracy to a refinement kernel that has no per-instance variant).  MPCB_E_INVALID: B > max_batch,
 * a negative stride, a missing x0, xbar, ubar, xref, uref, u0 or status.
 * Out of scope: the 17/6 model (mpcb_solve_iterate_pw17 below), rollout mode (mpcb_solve),
 * mpcb_eval and mpcb_solve_gains at per-instance weights, fp32 with the input box, an
 * interior-point fallback, the acados facade.
 */
int mpcb_solve_iterate_pw(mpcb_handle* h, int64_t B,
                          const void* x0, int64_t x0_sb,
                          const void* xbar, const void* ubar,
                          const void* xref, int64_t xref_sb,
                          const void* uref, int64_t uref_sb,
                          const void* wind, int64_t wind_sb,
                          const void* Qw, int64_t Qw_sb,
                          const void* Rw, int64_t Rw_sb,
                          const void* QNw, int64_t QNw_sb,
                          void* u0, void* X, void* U, int32_t* status, void* hip_stream);

/*
 * mpcb_solve_iterate_pw with a vehicle per instance (12/4 model): the QP of mpcb_solve_iterate_pw at
 * (xbar, ubar) with instance b's own mass, arms, yaw coefficient, T_blast and inertia (the model
 * record, MPCB_MODEL_REC above) in the RK4 rollout, the gaps and the sensitivities.  For a
 * controller whose belief about the vehicle differs per instance: an estimated payload, a tank that
 * empties in flight, B candidate vehicles in one batch.
 *   model, model_sb   the records, by the rules at MPCB_MODEL_REC; NULL = the handle's model, the
 *                     kernels of mpcb_solve_iterate_pw and its bits
 *   Qw, Rw, QNw and every other argument: as for mpcb_solve_iterate_pw, NULL and stride rules
 *   included; per-instance weights and a per-instance model combine freely
 * The statuses, the NaN rule (the record's 14 entries join it: an instance with a non-finite entry
 * gets MPCB_STATUS_NAN and NaN in u0, X and U, the others keep their bits), the input box (fp64
 * only, the plain active set with its cap, no interior-point hand-over), the aliasing of X / U with
 * xbar / ubar, the alignment rules and the first-call workspace (shared with
 * mpcb_solve_iterate_pw) are those of mpcb_solve_iterate_pw.  The same kernel with the instance's
 * vehicle held in LDS (fp64, 24 values) or in its lanes' registers (fp32).
 * MPCB_E_UNSUPPORTED: a 17/6 handle; an fp32 handle with box_u.  MPCB_E_INVALID: as for
 * mpcb_solve_iterate_pw, and a model stride that is negative or between 1 and MPCB_MODEL_REC - 1.
 */
int mpcb_solve_iterate_pm(mpcb_handle* h, int64_t B,
                          const void* x0, int64_t x0_sb,
                          const void* xbar, const void* ubar,
                          const void* xref, int64_t xref_sb,
                          const void* uref, int64_t uref_sb,
                          const void* wind, int64_t wind_sb,
                          const void* Qw, int64_t Qw_sb,
                          const void* Rw, int64_t Rw_sb,
                          const void* QNw, int64_t QNw_sb,
                          const void* model, int64_t model_sb,
                          void* u0, void* X, void* U, int32_t* status, void* hip_stream);

/*
 * mpcb_solve_gains with a vehicle per instance (12/4 model): K_k and P_0 of the LQ problem that
 * mpcb_solve_iterate_pm solves with the handle's weights, i.e. the recursion documented at
 * mpcb_solve_gains with [A_k | B_k] the RK4 sensitivities of instance b's vehicle.
 *   model, model_sb   the records, by the rules at MPCB_MODEL_REC; NULL = the handle's model, the
 *                     kernels of mpcb_solve_gains and its bits
 *   every other argument: as for mpcb_solve_gains on a 12/4 handle
 * The weights are the handle's: there is no per-instance-weight variant of the gains.  The mask
 * rules (fixed, or U on an input-box handle), the N <= 64 limit for fixed, the statuses (a
 * non-finite record entry: MPCB_STATUS_NAN and NaN outputs for that instance alone), the bitwise
 * symmetric P0, the exactly-zero rows of clamped components and the first-call workspace (shared
 * with mpcb_solve_gains) are as documented there.
 * MPCB_E_UNSUPPORTED on a 17/6 handle.  MPCB_E_INVALID: as for mpcb_solve_gains, and a model stride
 * that is negative or between 1 and MPCB_MODEL_REC - 1.
 */
int mpcb_solve_gains_pm(mpcb_handle* h, int64_t B,
                        const void* xbar, const void* ubar,
                        const void* U, const uint8_t* fixed,
                        const void* wind, int64_t wind_sb,
                        const void* model, int64_t model_sb,
                        void* K, void* P0, int32_t* status, void* hip_stream);

/*
 * mpcb_solve_vjp_w at per-instance weights: the product and the weight gradients of a
 * mpcb_solve_iterate_pw step.  The arguments are those of mpcb_solve_vjp_w plus the six weight
 * arguments of mpcb_solve_iterate_pw (NULL = the handle's matrix, strides as there, symmetric
 * matrices).  The formulas, the symmetry convention, the NaN rule (the weights join it), the
 * statuses and the active-set rule on U are those of mpcb_solve_vjp_w with instance b's matrices
 * in place of the handle's.  gQ, gR and gQN are per instance as before; for weights that differ
 * per instance they are the gradient itself and need no sum over B (for a broadcast matrix the
 * caller sums).  Both dtypes, with and without the input box (the set is read from U, so an fp32
 * handle with box_u is accepted here).  Without a weight output X, xref and uref are not read.
 * mpcb_solve_vjp and mpcb_solve_vjp_w launch the kernels they always did.
 * MPCB_E_UNSUPPORTED on a 17/6 handle; MPCB_E_INVALID as for mpcb_solve_vjp_w, and for a negative
 * weight stride.
 */
int mpcb_solve_vjp_pw(mpcb_handle* h, int64_t B,
                      const void* xbar, const void* ubar,
                      const void* X, const void* U,
                      const void* xref, int64_t xref_sb,
                      const void* uref, int64_t uref_sb,
                      const void* wind, int64_t wind_sb,
                      const void* Qw, int64_t Qw_sb,
                      const void* Rw, int64_t Rw_sb,
                      const void* QNw, int64_t QNw_sb,
                      const void* gX, const void* gU,
                      void* gx0, void* gxref, void* guref,
                      void* gQ, void* gR, void* gQN,
                      int32_t* status, void* hip_stream);

/*
 * mpcb_solve_iterate with the cost weights given per instance, on the 17/6 model: the QP of
 * mpcb_solve_iterate on a 17/6 handle in which instance b's own Q [17,17], R [6,6] and QN [17,17]
 * stand in place of the handle's (the stage cost stays s Q_b, s R_b; the terminal cost is QN_b).
 * The parameters (mpcb_set_params), the boxes, max_as_iter, dt and the model come from the handle.
 *   Qw, Qw_sb, Rw, Rw_sb, QNw, QNw_sb   by the rules of mpcb_solve_iterate_pw: DEVICE arrays of the
 *        handle's dtype, row-major; element strides, 0 broadcasts, a stride may exceed the record (the
 *        pad is never read), a negative stride is MPCB_E_INVALID; NULL = the handle's own matrix;
 *        element alignment only; symmetry (and definiteness) is the caller's contract.
 *   every other argument, the aliasing and the alignment rules: as for mpcb_solve_iterate (no wind)
 * Both dtypes, and every box mode the handle was created with: none, the input box (Mehrotra in
 * fp64, adaptive centring in fp32), the input and state box (fp64, with its polish).  The interior
 * point is the code of mpcb_solve_iterate, so MPCB_STATUS_MINSTEP and MPCB_STATUS_MAXITER mean what
 * they mean there.  An instance with a non-finite entry in its weights gets MPCB_STATUS_NAN and NaN
 * in u0, X and U; the other instances keep their bits.
 * The call runs the handle's own solve pipeline in the handle's workspace and chunks (nothing is
 * allocated), with the Riccati kernel's per-instance variant: each 16-lane group keeps its
 * instance's s Q_b, s R_b in its own LDS block.  It writes neither the QP statistics nor the
 * record of mpcb_last_kernels / mpcb_last_timing.  With all three pointers NULL it launches the
 * kernels of mpcb_solve_iterate and returns its bits.
 * MPCB_E_UNSUPPORTED on a 12/4 handle (mpcb_solve_iterate_pw is its counterpart, and keeps refusing
 * a 17/6 handle).  MPCB_E_INVALID: as for mpcb_solve_iterate, and a negative weight stride.  A
 * refused call writes nothing.
 * Out of scope: gains and mpcb_eval at per-instance weights, rollout mode, the acados facade,
 * per-instance boxes.
 */
int mpcb_solve_iterate_pw17(mpcb_handle* h, int64_t B,
                            const void* x0, int64_t x0_sb,
                            const void* xbar, const void* ubar,
                            const void* xref, int64_t xref_sb,
                            const void* uref, int64_t uref_sb,
                            const void* Qw, int64_t Qw_sb,
                            const void* Rw, int64_t Rw_sb,
                            const void* QNw, int64_t QNw_sb,
                            void* u0, void* X, void* U, int32_t* status, void* hip_stream);

/*
 * mpcb_solve_vjp17 at per-instance weights: the product and the weight gradients of a
 * mpcb_solve_iterate_pw17 step.  The arguments are those of mpcb_solve_vjp17 plus the six weight
 * arguments of mpcb_solve_iterate_pw17 (same rules).  Instance b's matrices stand in the adjoint
 * problem: gxref_k = s Q_b dx_k, gxref_N = QN_b dx_N, guref_k = s R_b du_k; gQ, gR and gQN by the
 * formulas of mpcb_solve_vjp17, per instance (for weights that differ per instance they are the
 * gradient itself; for a broadcast matrix the caller sums).  The active set as the `fixed` mask,
 * the workspace, the chunks, the statuses, the refusal of a state-box handle and the NaN rule (the
 * weights join it) are those of mpcb_solve_vjp17.  With all three weight pointers NULL it launches
 * the kernels of mpcb_solve_vjp17 and returns its bits.
 * MPCB_E_UNSUPPORTED on a 12/4 handle and on a box_x handle; MPCB_E_INVALID as for
 * mpcb_solve_vjp17, and for a negative weight stride.  A refused call writes nothing.
 */
int mpcb_solve_vjp_pw17(mpcb_handle* h, int64_t B,
                        const void* xbar, const void* ubar, const uint8_t* fixed,
                        const void* X, const void* U,
                        const void* xref, int64_t xref_sb,
                        const void* uref, int64_t uref_sb,
                        const void* Qw, int64_t Qw_sb,
                        const void* Rw, int64_t Rw_sb,
                        const void* QNw, int64_t QNw_sb,
                        const void* gX, const void* gU,
                        void* gx0, void* gxref, void* guref,
                        void* gQ, void* gR, void* gQN,
                        int32_t* status, void* hip_stream);

/*
 * The 17/6 product with active state rows: mpcb_solve_vjp17 / mpcb_solve_vjp_pw17 through the state
 * box (fp64).  The arguments are those of mpcb_solve_vjp_pw17 (each weight pointer may be NULL = the
 * handle's matrix; all three NULL = the handle's weights) and
 *   fixed_x [B,N+1,17] uint8   nonzero = state row (k, i) is active; stages 0 and N are never read
 *                              (the solver's state box covers stages 1..N-1).  As with `fixed` the
 *                              caller derives the set, by a tolerance on X - lbx and ubx - X
 *                              (BatchedMPC.active_mask17x; the polish of the state-box solve leaves an
 *                              active row within 1e-10 of its bound).
 * The adjoint problem gains one family of constraints, dx_k[i] = 0 on every active row (k, i),
 * 1 <= k <= N-1, beside dx_0 = 0, the dynamics and du_{k,m} = 0 on the clamped inputs.  With mu_k[i]
 * the multipliers of those rows (zero elsewhere) the outputs are gxref_k = s Q dx_k,
 * gxref_N = QN dx_N, guref_k = s R du_k, gx0 = nu_0 from nu_N = gX_N - QN dx_N,
 * nu_k = gX_k - s Q dx_k - mu_k + A_k^T nu_{k+1}, and gQ, gR, gQN by the unchanged formulas on this
 * (dx, du).  That is J^T (gX, gU) of the polished state-box solve on its active set: the polish
 * returns the exact solution of the equality-constrained QP on that set, whose KKT matrix is
 * symmetric.  The product is exact for the masks it is given, on every fp64 17/6 handle with or
 * without box_u / box_x.
 * Method: augmented-Lagrangian passes, as in the solver's own polish.  A pass is the Riccati
 * recursion of mpcb_solve_vjp17 with a penalty of 1e8 on the diagonal of every active row and the
 * multiplier estimates nu_k (zero at the start) in its gradient, then the forward pass; with
 * eq = max |dx_k[i]| over the active rows the instance is finished at eq <= 1e-10 max(1, |dx|_inf),
 * otherwise nu_k[i] += 1e8 dx_k[i] and it runs again, at most 12 passes.
 * status[B]: MPCB_STATUS_OK; MPCB_STATUS_NAN (the NaN rule of mpcb_solve_vjp17; the mask bytes
 * cannot be non-finite); MPCB_STATUS_QP_FAIL (a masked input Hessian is not positive definite);
 * MPCB_STATUS_MAXITER: not converged after 12 passes, the outputs are the last pass's.  That marks
 * a (nearly) dependent active set, rows that the free inputs cannot hold at zero independently,
 * at which the solve is not differentiable; no penalty makes such an instance converge.  An
 * instance without active rows finishes after one pass with the value of mpcb_solve_vjp17.
 * fixed_x == NULL: the call launches the kernels of mpcb_solve_vjp17 (all weight pointers NULL) or
 * mpcb_solve_vjp_pw17 and returns their bits, on a box_x handle too, where it means "no state row
 * is active, as the caller has checked".
 * The chunks, the first-call workspace (shared with mpcb_solve_vjp17) and the bit-reproducibility
 * without atomics are those of mpcb_solve_vjp17.
 * MPCB_E_UNSUPPORTED on a 12/4 handle and on an fp32 handle (a penalty of 1e8 has no meaning in
 * fp32, and an fp32 handle cannot have box_x); MPCB_E_INVALID as for mpcb_solve_vjp_pw17.  A refused
 * call writes nothing.
 * Out of scope: mpcb_solve_gains with state rows (a feedback law under state equalities is another
 * object), fp32, the 12/4 model, rollout mode.
 */
int mpcb_solve_vjp17_sx(mpcb_handle* h, int64_t B,
                        const void* xbar, const void* ubar,
                        const uint8_t* fixed, const uint8_t* fixed_x,
                        const void* X, const void* U,
                        const void* xref, int64_t xref_sb,
                        const void* uref, int64_t uref_sb,
                        const void* Qw, int64_t Qw_sb,
                        const void* Rw, int64_t Rw_sb,
                        const void* QNw, int64_t QNw_sb,
                        const void* gX, const void* gU,
                        void* gx0, void* gxref, void* guref,
                        void* gQ, void* gR, void* gQN,
                        int32_t* status, void* hip_stream);

/*
 * Plant integrator: x_out[b] = Phi(x[b], u[b]) with step T (one RK4 step).  Replaces
 * AcadosSimSolver set('x')/set('u')/solve()/get('x') (simulation_blaster.py:94-104).
 */
int mpcb_sim_step(mpcb_handle* h, int64_t B, const void* x, const void* u, const void* wind,
                  int64_t wind_sb, double T, void* x_out, void* hip_stream);

/*
 * mpcb_sim_step with a vehicle per instance (12/4 model): x_out[b] = Phi_b(x[b], u[b]), one RK4
 * step of instance b's own vehicle (the model record, MPCB_MODEL_REC above).  The plant of a
 * vehicle-parameter Monte Carlo: the truth each instance flies, whatever the controller believes.
 *   model, model_sb   the records, by the rules at MPCB_MODEL_REC; NULL = mpcb_sim_step itself
 *   every other argument: as for mpcb_sim_step
 * There is no status: an instance with a non-finite record entry gets NaN in its whole x_out row,
 * the other instances are unaffected.  A kernel of its own; mpcb_sim_step launches what it always did.
 * MPCB_E_UNSUPPORTED on a 17/6 handle (its per-instance data are mpcb_set_params).  MPCB_E_INVALID:
 * as for mpcb_sim_step, and a model stride that is negative or between 1 and MPCB_MODEL_REC - 1.
 */
int mpcb_sim_step_pm(mpcb_handle* h, int64_t B, const void* x, const void* u, const void* wind,
                     int64_t wind_sb, const void* model, int64_t model_sb, double T, void* x_out,
                     void* hip_stream);

/*
 * Reverse mode of the plant step (12/4 model, both dtypes).  With x_out = Phi_b(x, u) the step of
 * mpcb_sim_step_pm (of mpcb_sim_step when model == NULL) and gxn [B,12] the cotangent of x_out:
 *   gx     [B,12] = (d x_out / d x)^T gxn
 *   gu     [B,4]  = (d x_out / d u)^T gxn
 *   gwind  [B,3]  = (d x_out / d wind)^T gxn
 *   gmodel [B,14] = (d x_out / d record)^T gxn, in the order of MPCB_MODEL_REC
 * One sweep back through the four RK4 stages: the exact derivative of the discrete RK4 map, not of
 * the ODE.
 *   x, u, wind, wind_sb, model, model_sb, T   by the rules of mpcb_sim_step_pm
 *   gxn       required
 *   gx, gu, gwind, gmodel   any may be NULL (not computed), but not all four; contiguous rows,
 *             element alignment only.  gx may alias gxn (each instance's inputs are read before its
 *             outputs are written); no other aliasing is allowed.
 * Broadcast inputs: wind_sb == 0 or model_sb == 0 still gives per-instance gwind / gmodel rows; the
 * caller sums them (the convention of gQ).  wind == NULL is wind 0, and gwind is still valid.
 * model == NULL is the handle's vehicle: gmodel is then the gradient at the record equal to the
 * handle's config, and agrees to rounding with the call given that record broadcast.
 * gmodel: entry 0 is d/d mass; entries 5..13 are the nine entries of J taken as independent, through
 * both J and its inverse (gJ - Jinv^T gJinv Jinv^T, that product in fp64), so a symmetric
 * parametrisation adds (i,j) and (j,i).  No gradient is given with respect to gravity or T.
 * There is no status, as in mpcb_sim_step_pm: an instance with a non-finite entry in x, u, gxn, its
 * wind or its record gets NaN in every requested output row; the other instances keep their bits.
 * No atomics: the same call returns the same bits.
 * MPCB_E_UNSUPPORTED on a 17/6 handle.  MPCB_E_INVALID: B > max_batch, a missing x, u or gxn, all
 * four outputs NULL, a negative stride, 0 < model_sb < MPCB_MODEL_REC, T <= 0.  A refused call
 * writes nothing.
 */
int mpcb_sim_step_vjp(mpcb_handle* h, int64_t B,
                      const void* x, const void* u,
                      const void* wind, int64_t wind_sb,
                      const void* model, int64_t model_sb,
                      double T, const void* gxn,
                      void* gx, void* gu, void* gwind, void* gmodel,
                      void* hip_stream);

/*
 * mpcb_sim_step on the 17/6 model with the plant's parameters as an argument: x_out[b] =
 * Phi(x[b], u[b]; p_b), one RK4 step of f17.  The plant's truth given apart from the controller's
 * belief (mpcb_set_params): the 17/6 counterpart of `model` in mpcb_sim_step_pm.
 *   params, params_sb   DEVICE array [B|1, 25] of the handle's dtype in the vector layout of
 *             mpcb_set_params; instance b's vector starts at params + b * params_sb (elements).
 *             params_sb == 0 broadcasts one vector; params_sb >= 25 is allowed and the pad elements
 *             are never read; element alignment only.  NULL = mpcb_sim_step itself: the handle's
 *             mpcb_set_params array at stage 0 with its stride and its count check, or the defaults.
 *   every other argument: as for mpcb_sim_step (without the wind, a 12/4 extension)
 * The kernel of mpcb_sim_step with the caller's pointer: the bits of mpcb_set_params(those rows)
 * followed by mpcb_sim_step.  MPCB_E_UNSUPPORTED on a 12/4 handle.  MPCB_E_INVALID: as for
 * mpcb_sim_step, and a parameter stride that is negative or between 1 and 24.
 */
int mpcb_sim_step_p17(mpcb_handle* h, int64_t B, const void* x, const void* u,
                      const void* params, int64_t params_sb, double T, void* x_out, void* hip_stream);

/*
 * Reverse mode of the 17/6 plant step (both dtypes).  With x_out = Phi(x, u; p) the step of
 * mpcb_sim_step_p17 and gxn [B,17] the cotangent of x_out:
 *   gx      [B,17] = (d x_out / d x)^T gxn
 *   gu      [B,6]  = (d x_out / d u)^T gxn
 *   gparams [B,25] = (d x_out / d p)^T gxn, in the parameter vector's own column-major order
 *                    (mpcb_set_params); entry 24 is d/d T_blast
 * One sweep back through the four RK4 stages: the exact derivative of the discrete RK4 map, not of
 * the ODE.
 *   x, u, params, params_sb, T   by the rules of mpcb_sim_step_p17
 *   gxn       required
 *   gx, gu, gparams   any may be NULL (not computed), but not all three; contiguous rows, element
 *             alignment only.  gx may alias gxn (each instance's inputs are read before its outputs
 *             are written); no other aliasing is allowed.
 * Broadcast params (params_sb == 0, or NULL with a broadcast mpcb_set_params array or the defaults)
 * still gives per-instance gparams rows; the caller sums them (the convention of gQ and gmodel).
 * No gradient is given with respect to mass, J, the arms, gravity or T: those are the handle's.
 * There is no status: an instance with a non-finite entry in x, u, gxn or its parameter vector gets
 * NaN in every requested output row; the other instances keep their bits.  No atomics: the same
 * call returns the same bits.
 * MPCB_E_UNSUPPORTED on a 12/4 handle (mpcb_sim_step_vjp is its counterpart, and keeps refusing a
 * 17/6 handle).  MPCB_E_INVALID: B > max_batch, a missing x, u or gxn, all three outputs NULL, a
 * parameter stride that is negative or between 1 and 24, T <= 0, params == NULL with a non-broadcast
 * mpcb_set_params array shorter than B.  A refused call writes nothing.
 * (Weight gradients through a 17/6 closed loop come from mpcb_solve_vjp_pw17, which takes the
 * weights as arguments instead of installing them on the handle.)
 * Out of scope: stage-varying plant parameters (the plant step has one stage); gradients with respect to
 * the controller's mpcb_set_params; rollout mode.  (The state box: the solve's side of such a loop
 * is mpcb_solve_vjp17_sx; the plant step itself has no box.)
 */
int mpcb_sim_step_vjp17(mpcb_handle* h, int64_t B,
                        const void* x, const void* u,
                        const void* params, int64_t params_sb,
                        double T, const void* gxn,
                        void* gx, void* gu, void* gparams,
                        void* hip_stream);

/*
 * Synthetic inputs (SURVEY §8 d): Philox4x32-10 keyed by (seed, id_offset + i).
 *   ref_kind 0 = hover reference, 1 = per-instance sinusoid (c3);  wind may be NULL.
 * Writes x0 [B,nx], xref [B,N+1,nx] (or [1,...] if ref_kind==0 and xref_sb==0), uref likewise.
 */
int mpcb_gen_inputs(mpcb_handle* h, int64_t B, uint64_t seed, uint64_t id_offset, int ref_kind,
                    void* x0, void* xref, int64_t xref_sb, void* uref, int64_t uref_sb,
                    void* wind, void* hip_stream);

/*
 * Model parameters of the full 17/6 model (nx == 17): acados ``ocp_solver.set(k, 'p', p)``,
 * stage by stage (simulation_blaster.py:65-69; the vector layout of blastermodel.py:203-210:
 * column-major vec of J_angles 3x2, J_euler 3x3, J_p 3x3, then T_blast).
 *   params     DEVICE array; the 25-vector of instance b at stage k starts at
 *              params[b * params_sb + k * params_kb] (elements).  params_sb == 0: one row for
 *              every instance; params_kb == 0: the same vector on every stage 0..N-1 (the
 *              terminal stage has no dynamics).  mpcb_sim_step reads stage 0.
 *   count      instance rows the array holds: a later solve / linearize / sim_step of B > count
 *              instances fails with MPCB_E_INVALID unless params_sb == 0.
 * The caller keeps the array alive for those later calls.  NULL restores the defaults (zeros,
 * T_blast = mpcb_set_t_blast / cfg.t_blast, acados ``parameter_values``, blastermodel.py:280-282).
 * MPCB_E_UNSUPPORTED on a 12/4 handle (its only parameter is T_blast: mpcb_set_t_blast).
 */
int mpcb_set_params(mpcb_handle* h, int64_t count, const void* params, int64_t params_sb,
                    int64_t params_kb);

/*
 * T_blast, the blaster thrust p[24] (blastermodel.py:210), as a host scalar.  12/4 model: the
 * body-z force of the rigid-body slice for every instance and stage of later calls (replaces
 * ``set(k, 'p', p)`` with the Jacobian blocks zero; no re-creation of the handle).  17/6 model:
 * the default parameter vector's p[24] (used while no device parameters are set).  Waits for the
 * device (a configuration call, not a per-step one).
 */
int mpcb_set_t_blast(mpcb_handle* h, double t_blast);

/*
 * New cost weights for an existing handle: replaces acados ``cost_set(k, 'W', W)`` for a W that is
 * the same on all stages 0..N-1 (Q = W[:nx,:nx], R = W[nx:,nx:]) plus the terminal ``W_e`` (QN); no
 * re-creation of the handle or its workspace.  Q, R, QN are HOST arrays, row-major nx x nx, nu x nu
 * and nx x nx; NULL keeps the current matrix.  Every entry must be finite and each matrix symmetric
 * by the rule of mpcb_config; otherwise MPCB_E_INVALID and the handle is unchanged.  Updates the
 * handle's config and refills and uploads its whole weights block (every table derived from the
 * weights), on both models and every kernel path.  Waits for the device (a configuration call,
 * like mpcb_set_t_blast).  After any sequence of mpcb_set_t_blast, mpcb_set_params and
 * mpcb_set_weights calls the handle computes, bit for bit, what a handle created with the final
 * values computes.
 */
int mpcb_set_weights(mpcb_handle* h, const double* Q, const double* R, const double* QN);

/*
 * Point-of-contact Jacobians of the blaster stream for B vehicle poses (fp64, runs on the
 * current device / ``hip_stream``, no handle).  Replaces Jacobian_POC_Solver.solveJacobians
 * (src/scripts/Jacobian_POC_Solver.py:222-296, htm.py:7-36): stream ODE p' = v,
 * v' = -Mc v + g by RK4 with 10 steps, Newton ground-hit time (dT 1e-5, from 0.1, |z| <= 1e-3),
 * forward differences with eps 1e-6.
 *   pose   [B, 8]  phi, theta, psi, alpha1, alpha2, x, y, z (device)
 *   Mc     host double[9], the stream drag matrix (row-major; scalar M_c -> M_c I)
 *   poc [B,3], J_eul [B,3,3], J_mot [B,3,2], J_pos [B,3,3]; p25 [B,25] or NULL: the model
 *   parameter vector of blastermodel.py:203-210 (vec J_mot | vec J_eul | vec J_pos | t_blast)
 *   status [B]: 0, or MPCB_STATUS_MAXITER if a root solve hit max_iter
 */
int mpcb_poc_jacobians(int64_t B, const double* pose, double stream_velocity, const double* Mc,
                       int max_iter, double t_blast, double* poc, double* J_eul, double* J_mot,
                       double* J_pos, double* p25, int32_t* status, void* hip_stream);

/*
 * Work statistics of the last solve on an input-box handle.  12/4 (the active-set QP, c4): per
 * instance ``out[2b]`` = forward passes until its active set was the KKT point (including the
 * first, after the unconstrained Riccati pass) and ``out[2b+1]`` = backward stages its masked
 * Riccati passes recomputed (restarts skip the stages above the highest changed one); an instance
 * the active set handed to the interior point (mpcb_config.max_as_iter) adds its iterations to
 * ``out[2b]`` and N per iteration to ``out[2b+1]``.  17/6 (the
 * interior point): ``out[2b]`` = interior-point iterations (Newton directions computed),
 * ``out[2b+1]`` = polish passes (fp64 state box).  ``out`` is a DEVICE int32 array [B, 2], B <= that
 * solve's batch.  Reference counterpart: HPIPM's ``get_stats('qp_iter')``.  MPCB_E_UNSUPPORTED on
 * handles without an input box.
 * "The last solve" is the last accepted mpcb_solve or mpcb_solve_iterate: no other entry point
 * writes the statistics, so they survive any number of later calls of the others.  In particular
 * a boxed mpcb_solve_iterate_pw, mpcb_solve_iterate_pm or mpcb_solve_iterate_pw17 does not count
 * as a solve here: it keeps no statistics, and a read after it still returns those of the last
 * mpcb_solve / mpcb_solve_iterate, for at most that solve's batch (tests/test_gpu_history.py).
 */
int mpcb_qp_stats(mpcb_handle* h, int64_t B, int32_t* out, void* hip_stream);

/*
 * Quaternion helpers of utils/MathUtils.py (q = [w, x, y, z], MathUtils.py:9) for B pairs, fp64,
 * device arrays: prod[b] = q1[b] (x) q2[b] (quatMultiplication, :5-23), inv[b] = conj(q1[b])
 * (unitQuatInversion, :25-39), rot[b] = R(q1[b]) row-major 3x3 (quat2Rot, :41-54).  Any output
 * may be NULL; q2 may be NULL when prod is.  The reference evaluates them on CasADi SX and never
 * on the MPC path (imported at blastermodel.py:4).
 */
int mpcb_quat_ops(int64_t B, const double* q1, const double* q2, double* prod, double* inv,
                  double* rot, void* hip_stream);

/* Histogram of u0 per input channel over [lo, hi) into counts[nu][nbins] (int64, accumulated). */
int mpcb_histogram(mpcb_handle* h, int64_t B, const void* u0, double lo, double hi, int nbins,
                   int64_t* counts, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCB_H */
