// mpcb_gains.hip — the feedback gains K_k and the cost-to-go Hessian P_0 of the SQP_RTI step in
// iterate mode (mpcb_solve_gains, include/mpcb.h) for the 12/4 model (gfx950 / MI355X).
//
// The LQ problem that mpcb_solve_iterate solves at (xbar, ubar) has, with [A_k | B_k] the RK4
// sensitivities there, P_N = QN and for k = N-1 .. 0
//   H = blkdiag(sQ, sR) + [A|B]^T P_{k+1} [A|B],  K_k = -H~uu^-1 H~ux,  P_k = Hxx + Hux^T K_k,
// H~ the input blocks with the clamped components masked out (row and column of H_uu to 0, its
// diagonal to 1, the row of H_ux to 0).  Neither depends on gaps, references or linear terms.
//
// Layout of vjp_kernel (mpcb_vjp.hip): one wavefront = GROUPS (4) instances, an instance owns a
// 16-lane group, lane j owns direction j of (x, u).
//  * Pass 1 (nominal): lane j evaluates the RK4 stages k = j, j + 16, ... and publishes their
//    captured linearisation scalars; the same lanes build the stage bitmasks of the four input
//    components (bit k = clamped at stage k) from the `fixed` bytes or from U; the row ORs them.
//    Every input is read here, so the check sum of the NaN rule is complete before pass 2.
//  * Pass 2 (backward Riccati): vjp_kernel's stage body without any linear term; lane j < NX
//    holds column j of K_k and stores it straight to K in [nu, nx] order.  P_0 is stored from its
//    LDS copy after stage 0.  There is no forward pass.
// Stores to global memory carry no lane-divergent branch: an output nobody asked for, a padding
// group's and the input lanes' go to a sink in the wave's own workspace slot.  (LDS stores are
// predicated by lane where a lane owns the data: the rows of P, and with PM the group's model.)
#include <hip/hip_runtime.h>

#include <limits>

#include "../../include/mpcb.h"
#include "mpcb_common.h"
#include "mpcb_gains.h"

namespace mpcb {
namespace {

constexpr int SINK_K = 64 * NU;         // per slot: 16-lane rows of one stage's gains per group
constexpr int SINK_P = 64 * NX;         // per slot: a row of P_0 per lane

template <class T, int MASK, bool PM>
__global__ void __launch_bounds__(64) gains_kernel(GainsArgs<T> a) {
  __shared__ GroupLds<T> lds_all[GROUPS];
  // PM (mpcb_solve_gains_pm): the group's own vehicle, built in pass 1 from its record and kept for
  // the two passes in LDS (fp64) or in each lane's registers (fp32): pw_kernel's arrangement and
  // reasons (mpcb_pw.hip); otherwise the handle's
  constexpr bool PM_LDS = PM && sizeof(T) == 8;
  Model<T>* Mg = nullptr;
  if constexpr (PM_LDS) {
    __shared__ Model<T> m_all[GROUPS];
    Mg = &m_all[threadIdx.x >> 4];
  }
  const int lane = threadIdx.x;
  const int q = lane >> 4;
  const int j = lane & 15;
  const int jx = j < NX ? j : 0;       // clamped state index
  const int ju = j >= NX ? j - NX : 0; // clamped input index
  GroupLds<T>& L = lds_all[q];
  const int N = a.N;
  const T s = a.s;
  const Weights<T>& W = *a.W;
  T* slot = a.scratch + (int64_t)blockIdx.x * a.slot_elems;
  T* CC = slot;                                        // [N][GROUPS][LIN_STAGE] lin. scalars
  T* sinkK = CC + (int64_t)N * GROUPS * LIN_STAGE;     // [NU][64]
  T* sinkP = sinkK + SINK_K;                           // [64][NX]
  const T qnan = std::numeric_limits<T>::quiet_NaN();

  for (int64_t wave = blockIdx.x; wave * GROUPS < a.B; wave += gridDim.x) {
    const int64_t b_raw = wave * GROUPS + q;
    const bool valid = b_raw < a.B;
    const int64_t b = valid ? b_raw : a.B - 1;   // inactive groups recompute the last instance
    T chk = T(0);
    T w[3] = {T(0), T(0), T(0)};
    if (a.wind) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { w[i] = a.wind[b * a.wind_sb + i]; chk += w[i] * T(0); }
    }
    const T* xbp = a.xbar + b * (int64_t)(N + 1) * NX;
    const T* ubp = a.ubar + b * (int64_t)N * NU;
    // where this lane's stores go: lane j < NX owns column j of K_k and row j of P_0
    const bool outK = valid && a.K && j < NX, outP = valid && a.P0 && j < NX;
    T* const kp = outK ? a.K + b * (int64_t)N * (NU * NX) + jx : sinkK + lane;
    const int64_t kst = outK ? NU * NX : 0;      // stage stride
    const int krs = outK ? NX : 64;              // row stride
    T* const pp = outP ? a.P0 + b * (int64_t)(NX * NX) + jx * NX : sinkP + lane * NX;

    // ------------------------------------------------------------------ pass 1: nominal
    // (xbar_N is not read: no gap is formed and the terminal stage has no dynamics)
    uint64_t fix[NU];
#pragma unroll
    for (int m = 0; m < NU; ++m) fix[m] = 0;
    Model<T> Mi;   // PM: every lane derives the vehicle (the record's 14 values join the check sum);
                   // with PM_LDS lane 0 publishes it
    if constexpr (PM) {
      model_from_rec<T>(a.model + b * a.model_sb, a.M.g, Mi, chk);
      if constexpr (PM_LDS) {
        if (j == 0) *Mg = Mi;
        __syncthreads();
      }
    }
    const Model<T>& M = PM_LDS ? *Mg : (PM ? Mi : a.M);
    for (int k = j; k < N; k += 16) {
      T xb[NX], ub[NU], xn[NX];
      load_vec<NX>(xbp + (int64_t)k * NX, xb);
      load_vec<NU>(ubp + (int64_t)k * NU, ub);
#pragma unroll
      for (int i = 0; i < NX; ++i) chk += xb[i] * T(0);
#pragma unroll
      for (int m = 0; m < NU; ++m) chk += ub[m] * T(0);
      T* cc = CC + ((int64_t)k * GROUPS + q) * LIN_STAGE;
      rk4_nom<T>(xb, ub, a.h, M, w, xn, [&](int stage, const T* c) { store_vec<LIN_N>(cc + stage * LIN_N, c); });
      if constexpr (MASK) {
        if (a.fixed) {
          const uint8_t* fp = a.fixed + (b * (int64_t)N + k) * NU;
#pragma unroll
          for (int m = 0; m < NU; ++m) fix[m] |= (uint64_t)(fp[m] != 0 ? 1 : 0) << k;
        } else {
          // the active set of the solve that produced U (mpcb_solve_vjp's rule)
          const T* up = a.U + (b * (int64_t)N + k) * NU;
#pragma unroll
          for (int m = 0; m < NU; ++m) {
            const T u = up[m];
            chk += u * T(0);
            fix[m] |= (uint64_t)((u <= W.lbu[m] || u >= W.ubu[m]) ? 1 : 0) << k;
          }
        }
      }
    }
    if constexpr (MASK) {
#pragma unroll
      for (int m = 0; m < NU; ++m) {
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) fix[m] |= (uint64_t)__shfl_xor((unsigned long long)fix[m], d, 16);
      }
    }
    // every input has been read: the instance's check sum, the same in its 16 lanes
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) chk += __shfl_xor(chk, d, 16);
    const bool bad = chk != chk;
    if (j < NX) {
#pragma unroll
      for (int i = 0; i < NX; ++i) L.P[j * NX + i] = W.QN[i * NX + j];
    }
    __syncthreads();

    // ------------------------------------------------------------------ pass 2: Riccati
    bool qp_ok = true;
    for (int k = N - 1; k >= 0; --k) {
      T col[NX];
      {
        const T* cc = CC + ((int64_t)k * GROUPS + q) * LIN_STAGE;
        // tangent RK4 seeded with e_j: column j of [A|B]
        T dx[NX], du[NU];
#pragma unroll
        for (int i = 0; i < NX; ++i) dx[i] = (j == i) ? T(1) : T(0);
#pragma unroll
        for (int m = 0; m < NU; ++m) du[m] = (j == NX + m) ? T(1) : T(0);
        rk4_tan<T>(cc, dx, du, a.h, M, col);
      }
#pragma unroll
      for (int i = 0; i < NX; ++i) L.X[j * NX + i] = col[i];
      __syncthreads();
      // y = P col_j
      T y[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) y[i] = T(0);
#pragma unroll
      for (int l = 0; l < NX; ++l) {
        const T cl = col[l];
#pragma unroll
        for (int i = 0; i < NX; ++i) y[i] += L.P[l * NX + i] * cl;
      }
      // G[:, j] = [A|B]^T y  + s * blkdiag(Q, R)[:, j]
      T G[NZ];
#pragma unroll
      for (int i = 0; i < NZ; ++i) {
        T acc = T(0);
#pragma unroll
        for (int l = 0; l < NX; ++l) acc += L.X[i * NX + l] * y[l];
        G[i] = acc;
      }
      if (j < NX) {
#pragma unroll
        for (int i = 0; i < NX; ++i) G[i] += s * W.Q[i * NX + jx];
      } else {
#pragma unroll
        for (int n = 0; n < NU; ++n) G[NX + n] += s * W.R[n * NU + ju];
      }
#pragma unroll
      for (int m = 0; m < NU; ++m) L.Hu[j * NU + m] = G[NX + m];
      __syncthreads();   // all reads of L.X done; Hu visible
      T Ht[NU * NU], Hux_t[NU];
#pragma unroll
      for (int m = 0; m < NU; ++m) {
#pragma unroll
        for (int n = 0; n < NU; ++n) Ht[m * NU + n] = L.Hu[(NX + n) * NU + m];
        Hux_t[m] = G[NX + m];
      }
      // ---- masking (clamped components: du_m = 0)
      bool fixed[NU];
#pragma unroll
      for (int m = 0; m < NU; ++m) fixed[m] = false;
      if constexpr (MASK) {
#pragma unroll
        for (int m = 0; m < NU; ++m) {
          fixed[m] = (fix[m] >> k) & 1ull;
          Hux_t[m] = fixed[m] ? T(0) : Hux_t[m];
        }
#pragma unroll
        for (int m = 0; m < NU; ++m) {
#pragma unroll
          for (int n = 0; n < NU; ++n) {
            const bool f = fixed[m] || fixed[n];
            Ht[m * NU + n] = f ? ((m == n) ? T(1) : T(0)) : Ht[m * NU + n];
          }
        }
      }
      T Lc[10];
      chol4(Ht, Lc);
      bool ok = true;
#pragma unroll
      for (int i = 0; i < 10; ++i) ok = ok && (Lc[i] == Lc[i]);
      qp_ok = qp_ok && ok;
      T Kj[NU], nh[NU];
#pragma unroll
      for (int m = 0; m < NU; ++m) nh[m] = -Hux_t[m];
      chol4_solve(Lc, nh, Kj);
      if constexpr (MASK) {
        // a clamped row is +0, not the -0 the solve can leave from its right-hand side
#pragma unroll
        for (int m = 0; m < NU; ++m) Kj[m] = fixed[m] ? T(0) : Kj[m];
      }
      // P_new col j = G[0:12] + H_ux^T K[:, j] (unmasked H_ux: K's clamped rows are 0)
      T Pn[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        T acc = G[i];
#pragma unroll
        for (int m = 0; m < NU; ++m) acc += L.Hu[i * NU + m] * Kj[m];
        Pn[i] = acc;
      }
      // column j of K_k, rows m: K[b, k, m, j] (the input lanes' values go to the sink)
#pragma unroll
      for (int m = 0; m < NU; ++m) kp[k * kst + m * krs] = bad ? qnan : Kj[m];
      __syncthreads();   // everyone finished reading L.P / L.Hu
      // P_k symmetric by construction: entry (r, c) comes from lane max(r, c) (see solve_kernel)
      if (j < NX) {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          if (i <= j) L.P[j * NX + i] = Pn[i];
          if (i < j) L.P[i * NX + j] = Pn[i];
        }
      }
      __syncthreads();
    }

    // P_0 from its LDS copy, bitwise symmetric as stored there; row j by lane j
#pragma unroll
    for (int i = 0; i < NX; ++i) pp[i] = bad ? qnan : L.P[jx * NX + i];
    if (valid && j == 0)
      a.status[b] = bad ? MPCB_STATUS_NAN : (qp_ok ? MPCB_STATUS_OK : MPCB_STATUS_QP_FAIL);
    __syncthreads();   // the next wave of the stride rewrites the slot and L.P
  }
}

}  // namespace

int64_t gains_slot_elems(int N) { return (int64_t)N * (GROUPS * LIN_STAGE) + SINK_K + SINK_P; }

template <class T, bool PM> static hipError_t launch_gains_pm(const GainsArgs<T>& a, int grid, hipStream_t st) {
  if (a.mask)
    hipLaunchKernelGGL((gains_kernel<T, 1, PM>), dim3(grid), dim3(64), 0, st, a);
  else
    hipLaunchKernelGGL((gains_kernel<T, 0, PM>), dim3(grid), dim3(64), 0, st, a);
  return hipGetLastError();
}

// a.model == NULL: the instantiations of mpcb_solve_gains, whatever the caller
template <class T> hipError_t launch_gains(const GainsArgs<T>& a, int grid, hipStream_t st) {
  return a.model ? launch_gains_pm<T, true>(a, grid, st) : launch_gains_pm<T, false>(a, grid, st);
}

template hipError_t launch_gains<double>(const GainsArgs<double>&, int, hipStream_t);
template hipError_t launch_gains<float>(const GainsArgs<float>&, int, hipStream_t);

}  // namespace mpcb
