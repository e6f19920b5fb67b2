// mpcb_eval.hip — cost and KKT residuals of a given iterate (X, U) (mpcb_eval, include/mpcb.h).
//
// Per instance: the objective, the largest dynamics defect |Phi(x_k, u_k) - x_{k+1}|, the largest
// box violation and the natural residual of the reduced gradient.  The last needs the adjoint sweep
//   lambda_N = QN e_N,   g_k = s R eu_k + B_k^T lambda_{k+1},   lambda_k = s Q e_k + A_k^T lambda_{k+1}
// through the exact RK4 sensitivities, which maps onto the 16-lanes-per-instance layout of the
// linearisation kernels: lane j carries the unit tangent e_j through the RK4 step, so it holds
// column j of [A_k | B_k] and its dot product with lambda_{k+1} is component j of
// [A_k^T lambda ; B_k^T lambda].  A DPP row broadcast hands the new lambda to the 16 lanes.  No
// [A|B] is stored: the inputs and the four scalars are the only global traffic.
//
// Without res_stat no tangent is needed and the stages are independent (X is given): the
// *_stages kernel spreads the N + 1 stages of an instance over its 16 lanes.
//
// NaN rule: an instance with a non-finite input gets NaN in all outputs.  Every loaded input v
// adds v * 0 to a check sum (NaN unless v is finite), and the max reductions keep a NaN from
// either side (fmax would drop it), so a NaN born inside the arithmetic reaches the output too.
#include <hip/hip_runtime.h>

#include <limits>
#include <type_traits>

#include "../../include/mpcb.h"
#include "mpcb_common.h"
#include "mpcb_full.h"

namespace mpcb {
namespace {

template <class T> __device__ __forceinline__ T nanmax(T a, T b) { return (b > a || b != b) ? b : a; }
template <class T> __device__ __forceinline__ T absv(T v) { return v < T(0) ? -v : v; }

// reductions over the 16-lane row of an instance (fixed order: bitwise reproducible)
template <class T> __device__ __forceinline__ T row_sum(T v) {
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m, 16);
  return v;
}
template <class T> __device__ __forceinline__ T row_nanmax(T v) {
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) v = nanmax(v, __shfl_xor(v, m, 16));
  return v;
}

// |u - clip(u - g, lb, ub)|: the natural residual of one input component (|g| without the box)
template <class T> __device__ __forceinline__ T nat_res(T u, T g, T lb, T ub, int box) {
  if (!box) return absv(g);
  T z = u - g;
  z = z < lb ? lb : z;
  z = z > ub ? ub : z;
  return absv(u - z);
}
// the violation of lb <= v <= ub (0 inside)
template <class T> __device__ __forceinline__ T viol(T v, T lb, T ub) {
  return nanmax(nanmax(T(0), lb - v), v - ub);
}

template <class T>
__device__ __forceinline__ void write_out(const EvalArgs<T>& a, int64_t b, T chk, T cost, T ceq, T cin,
                                          T cst) {
  if (chk != chk) cost = ceq = cin = cst = std::numeric_limits<T>::quiet_NaN();
  if (a.cost) a.cost[b] = cost;
  if (a.res_eq) a.res_eq[b] = ceq;
  if (a.res_ineq) a.res_ineq[b] = cin;
  if (a.res_stat) a.res_stat[b] = cst;
}

// ------------------------------------------------------------------ 12/4, with res_stat
// The lane mapping of linearize_kernel: 4 instances per wave, lane j = direction j of [x; u].
template <class T>
__global__ void __launch_bounds__(64) eval_adjoint_kernel(EvalArgs<T> a) {
  const int lane = threadIdx.x, q = lane >> 4, j = lane & 15;
  const int64_t b = (int64_t)blockIdx.x * GROUPS + q;
  if (b >= a.B) return;
  const Weights<T>* W = reinterpret_cast<const Weights<T>*>(a.W);
  const int N = a.N;
  const bool sl = j < NX;             // state lane (else input lane j - NX)
  const int js = sl ? j : 0, ju = sl ? 0 : j - NX;
  const T* Xb = a.X + b * (int64_t)(N + 1) * NX;
  const T* Ub = a.U + b * (int64_t)N * NU;
  const T* xr = a.xref + b * a.xref_sb;
  const T* ur = a.uref + b * a.uref_sb;
  T chk = T(0);
  T w[3] = {T(0), T(0), T(0)};
  if (a.wind) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { w[i] = a.wind[b * a.wind_sb + i]; chk += w[i] * T(0); }
  }
  // the lane's row of the stage weight blkdiag(Q, R) (read again at every stage rather than held
  // across the RK4 tangent, which fills the register file), and its box
  const T* qrow = W->Q + js * NX;
  const T* rrow = W->R + ju * NU;
  const T lb = W->lbu[ju], ub = W->ubu[ju];
  // the unit tangent of the lane; also what picks the lane's own component out of a vector
  T dx[NX], du[NU];
#pragma unroll
  for (int i = 0; i < NX; ++i) dx[i] = (j == i) ? T(1) : T(0);
#pragma unroll
  for (int m = 0; m < NU; ++m) du[m] = (j == NX + m) ? T(1) : T(0);

  // terminal stage: lambda_N = QN e_N, component j on lane j
  // (xnj: component j of x_{k+1} on state lane j -- the lane checks its own component of the gap)
  T lam[NX];
  T v = T(0), ej = T(0), xnj = T(0);
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    const T xi = Xb[(int64_t)N * NX + i];
    const T ei = xi - xr[(int64_t)N * NX + i];
    chk += ei * T(0);
    v += W->QN[js * NX + i] * ei;
    ej += dx[i] * ei;
    xnj += dx[i] * xi;
  }
  v = sl ? v : T(0);
  T cost = T(0.5) * ej * v;
  static_for<NX>([&](auto i) { lam[i] = rowbc<decltype(i)::value>(v); });

  T ceq = T(0), cin = T(0), cst = T(0);
  for (int k = N - 1; k >= 0; --k) {
    T x[NX], u[NU], phi[NX], col[NX];
    // before the tangents: the lane's component of s blkdiag(Q, R) [e; eu], its own deviation ej
    // and (input lanes) its own input zo, so that only scalars stay live across the RK4
    T wq = T(0), wr = T(0), zo = T(0), xj = T(0);
    ej = T(0);
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      x[i] = Xb[(int64_t)k * NX + i];
      const T ei = x[i] - xr[(int64_t)k * NX + i];
      chk += ei * T(0);
      wq += qrow[i] * ei;
      ej += dx[i] * ei;
      xj += dx[i] * x[i];
    }
#pragma unroll
    for (int m = 0; m < NU; ++m) {
      u[m] = Ub[(int64_t)k * NU + m];
      const T em = u[m] - ur[(int64_t)k * NU + m];
      chk += em * T(0);
      wr += rrow[m] * em;
      ej += du[m] * em;
      zo += du[m] * u[m];
    }
    const T we = a.s * (sl ? wq : wr);
    cost += T(0.5) * ej * we;
    rk4<T, true>(x, dx, u, du, a.h, a.M, w, phi, col);
    T d = T(0), pj = T(0);
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      pj += dx[i] * phi[i];
      d += col[i] * lam[i];
    }
    ceq = nanmax(ceq, absv(pj - xnj));   // (0 - 0 on the input lanes)
    xnj = xj;
    v = we + d;   // lambda_k[j] on a state lane, g_k[j - NX] on an input lane
    if (!sl) {
      cst = nanmax(cst, nat_res(zo, v, lb, ub, a.box_u));
      if (a.box_u) cin = nanmax(cin, viol(zo, lb, ub));
    }
    static_for<NX>([&](auto i) { lam[i] = rowbc<decltype(i)::value>(v); });
  }
  if (a.x0 && sl) {
    const T x0j = a.x0[b * a.x0_sb + js];
    chk += x0j * T(0);
    ceq = nanmax(ceq, absv(xnj - x0j));
  }
  chk = row_sum(chk);
  ceq = row_nanmax(ceq);
  cost = row_sum(cost);
  cin = row_nanmax(cin);
  cst = row_nanmax(cst);
  if (j == 0) write_out(a, b, chk, cost, ceq, cin, cst);
}

// ------------------------------------------------------------------ 17/6, with res_stat
// lin17_packed yields every column of [A_k | B_k] in the 16-lane row (lanes 0..13 one RK4 tangent
// each, lanes 14 / 15 the nine closed-form columns); each lane keeps lambda . v per column it saw.
template <class T>
__global__ void __launch_bounds__(64) eval17_adjoint_kernel(EvalArgs<T> a) {
  const int lane = threadIdx.x, q = lane >> 4, t = lane & 15;
  const int64_t b = (int64_t)blockIdx.x * GQ17 + q;
  if (b >= a.B) return;
  const Weights17<T>* W = reinterpret_cast<const Weights17<T>*>(a.W);
  const int N = a.N;
  const T* Xb = a.X + b * (int64_t)(N + 1) * NX17;
  const T* Ub = a.U + b * (int64_t)N * NU17;
  const T* xr = a.xref + b * a.xref_sb;
  const T* ur = a.uref + b * a.uref_sb;
  const T* pb = a.p + b * a.p_sb;
  T chk = T(0), cost = T(0), ceq = T(0), cin = T(0), cst = T(0);
  T lam[NX17];
  {
    T e[NX17];
#pragma unroll
    for (int i = 0; i < NX17; ++i) {
      e[i] = Xb[(int64_t)N * NX17 + i] - xr[(int64_t)N * NX17 + i];
      chk += e[i] * T(0);
    }
#pragma unroll
    for (int i = 0; i < NX17; ++i) {
      T r = T(0);
#pragma unroll
      for (int l = 0; l < NX17; ++l) r += W->QN[i * NX17 + l] * e[l];
      lam[i] = r;
      cost += T(0.5) * e[i] * r;
    }
  }
  for (int k = N - 1; k >= 0; --k) {
    const T* xk = Xb + (int64_t)k * NX17;
    const T* uk = Ub + (int64_t)k * NU17;
    // the tangents first: only lambda is live across them (the RK4 tangent fills the register file)
    T acc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
    T gapk = T(0);
    lin17_packed<T>(t, pb + k * a.p_kb, a.h, a.M, xk, uk,
                    [&](int jc, const T* cv) {
                      T d = T(0);
#pragma unroll
                      for (int i = 0; i < NX17; ++i) d += cv[i] * lam[i];
                      // lane 14: columns 0..2 and 14..16 in slots 0..5; lane 15: columns 6..8 in
                      // slots 0..2; a tangent lane: its one column in slot 0
                      const int slot = jc < 3 ? jc : ((jc >= 14 && jc < 17) ? jc - 11 : ((jc >= 6 && jc < 9) ? jc - 6 : 0));
#pragma unroll
                      for (int sI = 0; sI < 6; ++sI) acc[sI] = (slot == sI) ? d : acc[sI];
                    },
                    [&](const T* phi) {   // (lane 0 holds the successor)
#pragma unroll
                      for (int i = 0; i < NX17; ++i) gapk = nanmax(gapk, absv(phi[i] - xk[NX17 + i]));
                    });
    ceq = nanmax(ceq, gapk);
    T al[NX17], bl[NU17];
    al[0] = rowbc<14>(acc[0]); al[1] = rowbc<14>(acc[1]); al[2] = rowbc<14>(acc[2]);
    al[3] = rowbc<0>(acc[0]); al[4] = rowbc<1>(acc[0]); al[5] = rowbc<2>(acc[0]);
    al[6] = rowbc<15>(acc[0]); al[7] = rowbc<15>(acc[1]); al[8] = rowbc<15>(acc[2]);
    al[9] = rowbc<3>(acc[0]); al[10] = rowbc<4>(acc[0]); al[11] = rowbc<5>(acc[0]);
    al[12] = rowbc<6>(acc[0]); al[13] = rowbc<7>(acc[0]);
    al[14] = rowbc<14>(acc[3]); al[15] = rowbc<14>(acc[4]); al[16] = rowbc<14>(acc[5]);
    bl[0] = rowbc<8>(acc[0]); bl[1] = rowbc<9>(acc[0]); bl[2] = rowbc<10>(acc[0]);
    bl[3] = rowbc<11>(acc[0]); bl[4] = rowbc<12>(acc[0]); bl[5] = rowbc<13>(acc[0]);
    T e[NX17], u[NU17], eu[NU17];
#pragma unroll
    for (int i = 0; i < NX17; ++i) {
      e[i] = xk[i] - xr[(int64_t)k * NX17 + i];
      chk += e[i] * T(0);
    }
#pragma unroll
    for (int m = 0; m < NU17; ++m) {
      u[m] = uk[m];
      eu[m] = u[m] - ur[(int64_t)k * NU17 + m];
      chk += eu[m] * T(0);
    }
    // Q e: lane t forms row t and the row broadcast hands the 16 to every lane; row 16 and R eu
    // are formed in every lane
    T qt = T(0), q16 = T(0);
#pragma unroll
    for (int l = 0; l < NX17; ++l) {
      qt += W->Q[t * NX17 + l] * e[l];
      q16 += W->Q[16 * NX17 + l] * e[l];
    }
    T c = e[16] * q16;
    static_for<16>([&](auto i) {
      const T qi = rowbc<decltype(i)::value>(qt);
      c += e[i] * qi;
      lam[i] = a.s * qi + al[i];
    });
    lam[16] = a.s * q16 + al[16];
#pragma unroll
    for (int m = 0; m < NU17; ++m) {
      T r = T(0);
#pragma unroll
      for (int l = 0; l < NU17; ++l) r += W->R[m * NU17 + l] * eu[l];
      c += eu[m] * r;
      if (a.box_u) cin = nanmax(cin, viol(u[m], W->lbu[m], W->ubu[m]));
      cst = nanmax(cst, nat_res(u[m], a.s * r + bl[m], W->lbu[m], W->ubu[m], a.box_u));
    }
    cost += T(0.5) * a.s * c;
  }
  ceq = row_nanmax(ceq);
  if (a.x0) {
#pragma unroll
    for (int i = 0; i < NX17; ++i) {
      const T x0i = a.x0[b * a.x0_sb + i];
      chk += x0i * T(0);
      ceq = nanmax(ceq, absv(Xb[i] - x0i));
    }
  }
  if (t == 0) write_out(a, b, chk, cost, ceq, cin, cst);
}

// ------------------------------------------------------------------ both models, without res_stat
// 16 lanes per instance, lane t takes the stages t, t + 16, ...; the row reduces.
template <class T, bool FULL>
__global__ void __launch_bounds__(64) eval_stages_kernel(EvalArgs<T> a) {
  constexpr int nx = FULL ? NX17 : NX, nu = FULL ? NU17 : NU;
  using WT = std::conditional_t<FULL, Weights17<T>, Weights<T>>;
  const int lane = threadIdx.x, q = lane >> 4, t = lane & 15;
  const int64_t b = (int64_t)blockIdx.x * GROUPS + q;
  if (b >= a.B) return;
  const WT* W = reinterpret_cast<const WT*>(a.W);
  const int N = a.N;
  const T* Xb = a.X + b * (int64_t)(N + 1) * nx;
  const T* Ub = a.U + b * (int64_t)N * nu;
  const T* xr = a.xref + b * a.xref_sb;
  const T* ur = a.uref + b * a.uref_sb;
  T chk = T(0), cost = T(0), ceq = T(0), cin = T(0);
  T w[3] = {T(0), T(0), T(0)};
  if constexpr (!FULL) {
    if (a.wind) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { w[i] = a.wind[b * a.wind_sb + i]; chk += w[i] * T(0); }
    }
  }
  for (int k = t; k <= N; k += 16) {
    T x[nx], e[nx];
#pragma unroll
    for (int i = 0; i < nx; ++i) {
      x[i] = Xb[(int64_t)k * nx + i];
      e[i] = x[i] - xr[(int64_t)k * nx + i];
      chk += e[i] * T(0);
    }
    const T* Wq = k < N ? W->Q : W->QN;
    T c = T(0);
#pragma unroll
    for (int i = 0; i < nx; ++i) {
      T r = T(0);
#pragma unroll
      for (int l = 0; l < nx; ++l) r += Wq[i * nx + l] * e[l];
      c += e[i] * r;
    }
    if (k < N) {
      T u[nu], phi[nx];
#pragma unroll
      for (int m = 0; m < nu; ++m) u[m] = Ub[(int64_t)k * nu + m];
#pragma unroll
      for (int m = 0; m < nu; ++m) {
        T r = T(0);
#pragma unroll
        for (int l = 0; l < nu; ++l) r += W->R[m * nu + l] * (u[l] - ur[(int64_t)k * nu + l]);
        const T eum = u[m] - ur[(int64_t)k * nu + m];
        chk += eum * T(0);
        c += eum * r;
        if (a.box_u) cin = nanmax(cin, viol(u[m], W->lbu[m], W->ubu[m]));
      }
      c *= a.s;
      if constexpr (FULL) {
        P17<T> P;
        unpack_p17(a.p + b * a.p_sb + k * a.p_kb, P);
        rk4_17<T, false>(x, nullptr, u, nullptr, a.h, a.M, P, phi, nullptr);
        if (a.box_x && k >= 1) {
#pragma unroll
          for (int i = 0; i < nx; ++i) cin = nanmax(cin, viol(x[i], W->lbx[i], W->ubx[i]));
        }
      } else {
        T dd[1];
        rk4<T, false>(x, nullptr, u, nullptr, a.h, a.M, w, phi, dd);
      }
#pragma unroll
      for (int i = 0; i < nx; ++i) ceq = nanmax(ceq, absv(phi[i] - Xb[(int64_t)(k + 1) * nx + i]));
    }
    if (k == 0 && a.x0) {
#pragma unroll
      for (int i = 0; i < nx; ++i) {
        const T x0i = a.x0[b * a.x0_sb + i];
        chk += x0i * T(0);
        ceq = nanmax(ceq, absv(x[i] - x0i));
      }
    }
    cost += T(0.5) * c;
  }
  chk = row_sum(chk);
  cost = row_sum(cost);
  ceq = row_nanmax(ceq);
  cin = row_nanmax(cin);
  if (t == 0) write_out(a, b, chk, cost, ceq, cin, T(0));
}

template <class T> unsigned eval_grid(const EvalArgs<T>& a) { return (unsigned)((a.B + GROUPS - 1) / GROUPS); }

}  // namespace

template <class T> hipError_t launch_eval(const EvalArgs<T>& a, hipStream_t st) {
  if (a.res_stat) hipLaunchKernelGGL((eval_adjoint_kernel<T>), dim3(eval_grid(a)), dim3(64), 0, st, a);
  else hipLaunchKernelGGL((eval_stages_kernel<T, false>), dim3(eval_grid(a)), dim3(64), 0, st, a);
  return hipGetLastError();
}
template <class T> hipError_t launch_eval17(const EvalArgs<T>& a, hipStream_t st) {
  if (a.res_stat) hipLaunchKernelGGL((eval17_adjoint_kernel<T>), dim3(eval_grid(a)), dim3(64), 0, st, a);
  else hipLaunchKernelGGL((eval_stages_kernel<T, true>), dim3(eval_grid(a)), dim3(64), 0, st, a);
  return hipGetLastError();
}

template hipError_t launch_eval<double>(const EvalArgs<double>&, hipStream_t);
template hipError_t launch_eval<float>(const EvalArgs<float>&, hipStream_t);
template hipError_t launch_eval17<double>(const EvalArgs<double>&, hipStream_t);
template hipError_t launch_eval17<float>(const EvalArgs<float>&, hipStream_t);

}  // namespace mpcb
