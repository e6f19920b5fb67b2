// mpcb_vjp.hip — vector-Jacobian product of the SQP_RTI step in iterate mode (mpcb_solve_vjp and
// mpcb_solve_vjp_w, include/mpcb.h) for the 12/4 model (gfx950 / MI355X).
//
// With the linearisation point (xbar, ubar) and the active set held fixed, (X, U) of
// mpcb_solve_iterate is an affine function of (x0, xref, uref).  The transpose of that map applied
// to the cotangents (gX, gU) is one more LQ solve over the same [A_k | B_k], weights and clamped
// components, with linear terms (-gX, -gU), no gaps and dx_0 = 0:
//   gxref_k = s Q dx_k (k < N),  gxref_N = QN dx_N,  guref_k = s R du_k,  gx0 = -p_0,
// p_0 the linear term of the value function at stage 0.
//
// Layout of solve_kernel (mpcb_solve.hip): one wavefront = GROUPS (4) instances, an instance owns
// a 16-lane group, lane j owns direction j of (x, u).
//  * Pass 1 (nominal): the stages of an iterate are independent (xbar is given, no gap is needed),
//    so lane j evaluates the RK4 stages k = j, j + 16, ... and publishes their captured
//    linearisation scalars.  With the box, the same lanes read U_k into the stage bitmasks of the
//    four input components (bit k = clamped at stage k); the row ORs them together.
//  * Pass 2 (backward Riccati): as solve_kernel's, lane j carrying column j of [A_k | B_k] as the
//    RK4 tangent seeded with e_j; the gradient of the stage is -g (lane j reads its own cotangent
//    component).  Clamped components are masked out of the 4x4 input Hessian.  Gains go to the slot
//    workspace; the pass ends with gx0.
//  * Pass 3 (forward): dx_0 = 0, du_k = K_k dx_k + kff_k, dx_{k+1} = the RK4 tangent along
//    (dx_k, du_k); lane j writes component j of s blkdiag(Q, R) (dx_k, du_k).
//
// NaN rule (mpcb_eval's): every loaded input v adds v * 0 to a check sum, NaN unless v is finite;
// an instance whose sum is NaN gets status NAN and NaN in every output.  All inputs are read
// before the first output is written.  The groups of a wave share nothing but the barriers.
#include <hip/hip_runtime.h>

#include <limits>

#include "../../include/mpcb.h"
#include "mpcb_common.h"
#include "mpcb_vjp.h"

namespace mpcb {
namespace {

constexpr int VJP_KR = 4;   // gain values per lane and stage: lane j < NX column j of K, lane NX+m kff[m]

// WG: also the weight gradients (mpcb_solve_vjp_w).  At a fixed linearisation point and active set
//   gQ = -s sym(sum_{k<N} dx_k rx_k^T),  gR = -s sym(sum_{k<N} du_k ru_k^T),  gQN = -sym(dx_N rx_N^T),
// rx_k = X_k - xref_k, ru_k = U_k - uref_k the residuals of the solve's output, sym(M) = (M + M^T)/2.
// Pass 3 holds (dx_k, du_k) in every lane: lane j < NX accumulates row j of the Q sum, lane NX + m
// row m of the R sum, per instance (the caller sums over the batch; no atomics).  X, U and the
// references are read in pass 1 by the lane that owns the stage, for the check sum, and again in
// pass 3.  The rows meet in LDS, where entry (r, c), c <= r, is formed once and stored to both places.
//
// PW: the weights are instance b's own (mpcb_solve_vjp_pw): Q, R and QN at a.Qw + b * a.Qw_sb and
// so on instead of the handle's block (the box still comes from there).  Lane j keeps column j of
// blkdiag(Q, R) in registers (the matrices are symmetric: also its row) and reads its column of QN
// where the terminal stage needs it; these loads join the check sum.  The other instantiations do
// not change.
template <class T, int BOX, int WG, int PW = 0>
__global__ void __launch_bounds__(64) vjp_kernel(VjpArgs<T> a) {
  __shared__ GroupLds<T> lds_all[GROUPS];
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
  T* KR = CC + (int64_t)N * GROUPS * LIN_STAGE;        // [N][64][VJP_KR]        gains

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
    // (PW) the lane's column of blkdiag(Q, R) and where its column of QN starts
    T wcol[NX];
    const T* qnp = nullptr;
    if constexpr (PW) {
      const T* Qp = a.Qw + b * a.Qw_sb;
      const T* Rp = a.Rw + b * a.Rw_sb;
      qnp = a.QNw + b * a.QNw_sb + jx;
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        wcol[i] = j < NX ? Qp[i * NX + jx] : (i < NU ? Rp[i * NU + ju] : T(0));
        chk += wcol[i] * T(0);
      }
    }
    const T* gXp = a.gX ? a.gX + b * (int64_t)(N + 1) * NX : nullptr;
    const T* gUp = a.gU ? a.gU + b * (int64_t)N * NU : nullptr;
    // (WG) the solve's output and its references
    const T* Xp = WG ? a.X + b * (int64_t)(N + 1) * NX : nullptr;
    const T* Up = WG ? a.U + b * (int64_t)N * NU : nullptr;
    const T* xrp = WG ? a.xref + b * a.xref_sb : nullptr;
    const T* urp = WG ? a.uref + b * a.uref_sb : nullptr;

    // ------------------------------------------------------------------ pass 1: nominal
    // (xbar_N is not read: no gap is formed and the terminal stage has no dynamics)
    uint64_t fix[NU];
#pragma unroll
    for (int m = 0; m < NU; ++m) fix[m] = 0;
    for (int k = j; k < N; k += 16) {
      T xb[NX], ub[NU], xn[NX];
      load_vec<NX>(xbp + (int64_t)k * NX, xb);
      load_vec<NU>(ubp + (int64_t)k * NU, ub);
#pragma unroll
      for (int i = 0; i < NX; ++i) chk += xb[i] * T(0);
#pragma unroll
      for (int m = 0; m < NU; ++m) chk += ub[m] * T(0);
      T* cc = CC + ((int64_t)k * GROUPS + q) * LIN_STAGE;
      rk4_nom<T>(xb, ub, a.h, a.M, w, xn, [&](int stage, const T* c) { store_vec<LIN_N>(cc + stage * LIN_N, c); });
      if constexpr (BOX) {
        // the active set of the solve that produced U: the box kernels write the bound itself
        const T* up = a.U + (b * (int64_t)N + k) * NU;
#pragma unroll
        for (int m = 0; m < NU; ++m) {
          const T u = up[m];
          chk += u * T(0);
          fix[m] |= (uint64_t)((u <= W.lbu[m] || u >= W.ubu[m]) ? 1 : 0) << k;
        }
      }
      if constexpr (WG) {
        // what pass 3 reads again for the residuals joins the check sum here (U: above with the box)
#pragma unroll
        for (int i = 0; i < NX; ++i) chk += Xp[(int64_t)k * NX + i] * T(0) + xrp[(int64_t)k * NX + i] * T(0);
#pragma unroll
        for (int m = 0; m < NU; ++m) chk += urp[(int64_t)k * NU + m] * T(0);
        if constexpr (!BOX) {
#pragma unroll
          for (int m = 0; m < NU; ++m) chk += Up[(int64_t)k * NU + m] * T(0);
        }
      }
    }
    if constexpr (WG) {
      if (j == 15) {   // the terminal stage, on the lane with the fewest stages
#pragma unroll
        for (int i = 0; i < NX; ++i) chk += Xp[(int64_t)N * NX + i] * T(0) + xrp[(int64_t)N * NX + i] * T(0);
      }
    }
    if constexpr (BOX) {
#pragma unroll
      for (int m = 0; m < NU; ++m) {
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) fix[m] |= (uint64_t)__shfl_xor((unsigned long long)fix[m], d, 16);
      }
    }
    __syncthreads();

    // ------------------------------------------------------------------ pass 2: Riccati
    T pj;       // p_{k+1}[j]
    {
      const T gN = (gXp && j < NX) ? gXp[(int64_t)N * NX + jx] : T(0);
      chk += gN * T(0);
      pj = -gN;
      if (j < NX) {
        if constexpr (PW) {
#pragma unroll
          for (int i = 0; i < NX; ++i) {
            const T v = qnp[i * NX];
            chk += v * T(0);
            L.P[j * NX + i] = v;
          }
        } else {
#pragma unroll
          for (int i = 0; i < NX; ++i) L.P[j * NX + i] = W.QN[i * NX + j];
        }
      }
      __syncthreads();
    }
    bool qp_ok = true;
    for (int k = N - 1; k >= 0; --k) {
      T col[NX];
      // the lane's own cotangent component: the stage gradient is -g
      T gj = T(0);
      if (j < NX) {
        if (gXp) gj = gXp[(int64_t)k * NX + jx];
      } else {
        if (gUp) gj = gUp[(int64_t)k * NU + ju];
      }
      chk += gj * T(0);
      {
        const T* cc = CC + ((int64_t)k * GROUPS + q) * LIN_STAGE;
        // tangent RK4 seeded with e_j: column j of [A|B]
        T dx[NX], du[NU];
#pragma unroll
        for (int i = 0; i < NX; ++i) dx[i] = (j == i) ? T(1) : T(0);
#pragma unroll
        for (int m = 0; m < NU; ++m) du[m] = (j == NX + m) ? T(1) : T(0);
        rk4_tan<T>(cc, dx, du, a.h, a.M, col);
        L.hv[j] = pj;
      }
#pragma unroll
      for (int i = 0; i < NX; ++i) L.X[j * NX + i] = col[i];
      __syncthreads();
      // h_j = col_j . p - g_j
      T hj = -gj;
#pragma unroll
      for (int l = 0; l < NX; ++l) hj += col[l] * L.hv[l];
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
      if constexpr (PW) {
        if (j < NX) {
#pragma unroll
          for (int i = 0; i < NX; ++i) G[i] += s * wcol[i];
        } else {
#pragma unroll
          for (int n = 0; n < NU; ++n) G[NX + n] += s * wcol[n];
        }
      } else if (j < NX) {
#pragma unroll
        for (int i = 0; i < NX; ++i) G[i] += s * W.Q[i * NX + jx];
      } else {
#pragma unroll
        for (int n = 0; n < NU; ++n) G[NX + n] += s * W.R[n * NU + ju];
      }
#pragma unroll
      for (int m = 0; m < NU; ++m) L.Hu[j * NU + m] = G[NX + m];
      __syncthreads();   // all reads of L.hv / L.X done; Hu visible
      L.hv[j] = hj;
      __syncthreads();
      T Ht[NU * NU], ht[NU], Hux_t[NU];
#pragma unroll
      for (int m = 0; m < NU; ++m) {
#pragma unroll
        for (int n = 0; n < NU; ++n) Ht[m * NU + n] = L.Hu[(NX + n) * NU + m];
        ht[m] = L.hv[NX + m];
        Hux_t[m] = G[NX + m];
      }
      // ---- input-box masking (clamped components: du_m = 0)
      if constexpr (BOX) {
        bool fixed[NU];
#pragma unroll
        for (int m = 0; m < NU; ++m) {
          fixed[m] = (fix[m] >> k) & 1ull;
          ht[m] = fixed[m] ? T(0) : ht[m];
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
      T kff[NU], Kj[NU], nh[NU];
#pragma unroll
      for (int m = 0; m < NU; ++m) nh[m] = -ht[m];
      chol4_solve(Lc, nh, kff);
#pragma unroll
      for (int m = 0; m < NU; ++m) nh[m] = -Hux_t[m];
      chol4_solve(Lc, nh, Kj);
      // p_new = h_x + H_ux^T kff (unmasked H_ux);  P_new col j = G[0:12] + H_ux^T K[:, j]
      T pn = hj;
#pragma unroll
      for (int m = 0; m < NU; ++m) pn += G[NX + m] * kff[m];
      T Pn[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        T acc = G[i];
#pragma unroll
        for (int m = 0; m < NU; ++m) acc += L.Hu[i * NU + m] * Kj[m];
        Pn[i] = acc;
      }
      T* rec = KR + ((int64_t)k * 64 + lane) * VJP_KR;
      if (j < NX) {
#pragma unroll
        for (int m = 0; m < NU; ++m) rec[m] = Kj[m];
      } else {
        rec[0] = sel<NU>(kff, ju);
      }
      __syncthreads();   // everyone finished reading L.P / L.Hu
      // P_k symmetric by construction: entry (r, c) comes from lane max(r, c) (see solve_kernel)
      if (j < NX) {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          if (i <= j) L.P[j * NX + i] = Pn[i];
          if (i < j) L.P[i * NX + j] = Pn[i];
        }
      }
      pj = pn;
      __syncthreads();
    }

    // every input has been read: the instance's check sum, the same in its 16 lanes
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) chk += __shfl_xor(chk, d, 16);
    const bool bad = chk != chk;
    const T qnan = std::numeric_limits<T>::quiet_NaN();
    if (valid && a.gx0 && j < NX) a.gx0[b * NX + j] = bad ? qnan : -pj;
    if (valid && j == 0)
      a.status[b] = bad ? MPCB_STATUS_NAN : (qp_ok ? MPCB_STATUS_OK : MPCB_STATUS_QP_FAIL);

    // ------------------------------------------------------------------ pass 3: forward
    // (the two pointers are read here in both variants: read inside the stage loop they would stand
    // among its loads in the weight variant only, see the note on operand order below)
    T* const gxrefp = a.gxref;
    T* const gurefp = a.guref;
    if (WG || gxrefp || gurefp) {
      T dxk[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) dxk[i] = T(0);
      // (WG) the lane's row of the running outer-product sums lives in LDS, which pass 2 is done
      // with: row j of the Q sum in L.P (state lanes), row m of the R sum in L.hv (input lanes);
      // the residual it multiplies is read through the lane's own pair of pointers
      const T* const zp = j < NX ? Xp : Up;
      const T* const rp = j < NX ? xrp : urp;
      const int zw = j < NX ? NX : NU;
      T* const wrow = j < NX ? &L.P[j * NX] : &L.hv[ju * NU];
      if constexpr (WG) {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          if (i < NU || j < NX) wrow[i] = T(0);
        }
      }
      for (int k = 0; k < N; ++k) {
        T duk[NU];
#pragma unroll
        for (int m = 0; m < NU; ++m) duk[m] = KR[((int64_t)k * 64 + q * 16 + NX + m) * VJP_KR];
#pragma unroll
        for (int l = 0; l < NX; ++l) {
          const T* r = KR + ((int64_t)k * 64 + q * 16 + l) * VJP_KR;
#pragma unroll
          for (int m = 0; m < NU; ++m) duk[m] += r[m] * dxk[l];
        }
        // component j of s blkdiag(Q, R) (dx_k, du_k)
        T acc = T(0);
        if constexpr (PW) {
          if (j < NX) {
#pragma unroll
            for (int i = 0; i < NX; ++i) acc += wcol[i] * dxk[i];
          } else {
#pragma unroll
            for (int n = 0; n < NU; ++n) acc += wcol[n] * duk[n];
          }
        } else if (j < NX) {
#pragma unroll
          for (int i = 0; i < NX; ++i) acc += W.Q[jx * NX + i] * dxk[i];
        } else {
#pragma unroll
          for (int n = 0; n < NU; ++n) acc += W.R[ju * NU + n] * duk[n];
        }
        const T v = bad ? qnan : s * acc;
        if (valid) {
          if (j < NX) {
            if (gxrefp) gxrefp[(b * (N + 1) + k) * NX + j] = v;
          } else {
            if (gurefp) gurefp[(b * N + k) * NU + ju] = v;
          }
        }
        const T* cc = CC + ((int64_t)k * GROUPS + q) * LIN_STAGE;
        T dphi[NX];
        rk4_tan<T>(cc, dxk, duk, a.h, a.M, dphi);
        if constexpr (WG) {
          // row j of dx_k rx_k^T (state lanes) / row m of du_k ru_k^T (input lanes: NU entries).
          // gxref and guref must keep the bits of the plain kernel, and the compiler decides which
          // product of a sum of two it fuses from the order of the operands, which its
          // reassociation pass takes from where the loads they descend from stand in the block.
          // So this comes behind everything the plain kernel does in a stage, keeps its sums in
          // LDS and not in registers, and reads du_k[ju] through an unrolled loop like the plain
          // kernel's own loops over duk: with sel<NU>(duk, ju) the array left memory earlier in
          // the pipeline in one instantiation, its loads left the block, and dx_{k+1} differed
          // in the last bit.  (Check: the optimised IR of the stage loop, operand for operand.)
          T zu = duk[0];
#pragma unroll
          for (int m = 1; m < NU; ++m) zu = (m == ju) ? duk[m] : zu;
          const T zj = j < NX ? sel<NX>(dxk, jx) : zu;
          const int64_t o = (int64_t)k * zw;
#pragma unroll
          for (int i = 0; i < NX; ++i) {
            if (i < NU || j < NX) wrow[i] += zj * (zp[o + i] - rp[o + i]);
          }
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) dxk[i] = dphi[i];
      }
      if (valid && gxrefp && j < NX) {
        T acc = T(0);
        if constexpr (PW) {
#pragma unroll
          for (int i = 0; i < NX; ++i) acc += qnp[i * NX] * dxk[i];
        } else {
#pragma unroll
          for (int i = 0; i < NX; ++i) acc += W.QN[jx * NX + i] * dxk[i];
        }
        gxrefp[(b * (N + 1) + N) * NX + j] = bad ? qnan : acc;
      }
      if constexpr (WG) {
        // the rows are in LDS; the terminal product joins them in L.X (stride NX)
        if (j < NX) {
          const T zj = sel<NX>(dxk, jx);
#pragma unroll
          for (int i = 0; i < NX; ++i)
            L.X[j * NX + i] = zj * (Xp[(int64_t)N * NX + i] - xrp[(int64_t)N * NX + i]);
        }
        __syncthreads();
        // symmetric by construction: entry (r, c), c <= r, is formed once by lane r and stored twice
        const T hs = T(-0.5) * s;
        if (j < NX) {
#pragma unroll
          for (int i = 0; i < NX; ++i) {
            if (i <= j && valid) {
              const T vq = bad ? qnan : hs * (L.P[j * NX + i] + L.P[i * NX + j]);
              const T vn = bad ? qnan : T(-0.5) * (L.X[j * NX + i] + L.X[i * NX + j]);
              if (a.gQ) {
                a.gQ[b * (NX * NX) + j * NX + i] = vq;
                a.gQ[b * (NX * NX) + i * NX + j] = vq;
              }
              if (a.gQN) {
                a.gQN[b * (NX * NX) + j * NX + i] = vn;
                a.gQN[b * (NX * NX) + i * NX + j] = vn;
              }
            }
          }
        } else {
#pragma unroll
          for (int n = 0; n < NU; ++n) {
            if (n <= ju && valid && a.gR) {
              const T vr = bad ? qnan : hs * (L.hv[ju * NU + n] + L.hv[n * NU + ju]);
              a.gR[b * (NU * NU) + ju * NU + n] = vr;
              a.gR[b * (NU * NU) + n * NU + ju] = vr;
            }
          }
        }
      }
    }
    __syncthreads();   // the next wave of the stride rewrites the slot
  }
}

}  // namespace

int64_t vjp_slot_elems(int N) { return (int64_t)N * (GROUPS * LIN_STAGE + 64 * VJP_KR); }

template <class T, int PW> static hipError_t launch_vjp_pw(const VjpArgs<T>& a, int grid, hipStream_t st) {
  const bool wg = a.gQ || a.gR || a.gQN;   // no weight gradient asked for: the plain kernels
  if (a.box && wg)
    hipLaunchKernelGGL((vjp_kernel<T, 1, 1, PW>), dim3(grid), dim3(64), 0, st, a);
  else if (wg)
    hipLaunchKernelGGL((vjp_kernel<T, 0, 1, PW>), dim3(grid), dim3(64), 0, st, a);
  else if (a.box)
    hipLaunchKernelGGL((vjp_kernel<T, 1, 0, PW>), dim3(grid), dim3(64), 0, st, a);
  else
    hipLaunchKernelGGL((vjp_kernel<T, 0, 0, PW>), dim3(grid), dim3(64), 0, st, a);
  return hipGetLastError();
}

// a.Qw: per-instance weights (mpcb_solve_vjp_pw: all three pointers are set)
template <class T> hipError_t launch_vjp(const VjpArgs<T>& a, int grid, hipStream_t st) {
  return a.Qw ? launch_vjp_pw<T, 1>(a, grid, st) : launch_vjp_pw<T, 0>(a, grid, st);
}

template hipError_t launch_vjp<double>(const VjpArgs<double>&, int, hipStream_t);
template hipError_t launch_vjp<float>(const VjpArgs<float>&, int, hipStream_t);

}  // namespace mpcb
