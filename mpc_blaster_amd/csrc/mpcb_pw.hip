// mpcb_pw.hip — the SQP_RTI step in iterate mode with cost weights per instance
// (mpcb_solve_iterate_pw, include/mpcb.h) for the 12/4 model (gfx950 / MI355X).
//
// The QP of mpcb_solve_iterate at (xbar, ubar), with instance b's own Q, R and QN in place of the
// handle's: one self-contained kernel of the family of vjp_kernel (mpcb_vjp.hip) and gains_kernel
// (mpcb_gains.hip); the tuned solve paths are not involved.
//
// Layout of vjp_kernel: one wavefront = GROUPS (4) instances, an instance owns a 16-lane group,
// lane j owns direction j of (x, u).
//  * Pass 1 (nominal): the stages of an iterate are independent, so lane j evaluates the RK4 stages
//    k = j, j + 16, ..., publishes their captured linearisation scalars and gaps and copies
//    (xbar_k, ubar_k) to the slot (X and U may alias xbar and ubar: nothing of them is read after
//    this pass).  The group stages its Q, R and QN in LDS (304 values).  Every input is read here,
//    so the check sum of the NaN rule is complete before pass 2.
//  * Pass 2 (backward Riccati): the masked stage of vjp_kernel with the solve's linear terms (gap,
//    s Q (xbar - xref), s R (ubar - uref)); a clamped component enters with du_m = bound - ubar_m
//    (oracle.ocp._masked_stage).  Gains go to the slot, with the box also the input rows of the
//    stage Hessian and h_u.
//  * Pass 3 (forward): dx_0 = x0 - xbar_0, du_k = K_k dx_k + k_k, dx_{k+1} = the RK4 tangent along
//    (dx_k, du_k) plus the gap; writes X = xbar + dx, U = ubar + du (a clamped component: the bound
//    itself).  With the box the input lanes evaluate the multipliers and the infeasible set V; the
//    set update is oracle.ocp.pdas_solve's (full exchange of V with the Kim-Park safeguard,
//    pbar = 3, and the least-index backup), and passes 2-3 repeat until every group of the wave
//    has stopped or the cap is reached.  There is no hand-over to an interior point.
// Stores to global memory carry no lane-divergent branch: a padding group's, a stopped group's and
// those of an output nobody asked for go to a sink in the wave's own workspace slot.  (LDS stores
// are predicated by lane where a lane owns the data: the rows of P, and with PM the group's model.)
//
// PM (mpcb_solve_iterate_pm): instance b's vehicle in place of the handle's.  Pass 1 first reads the
// group's 14-value record, derives minv and Jinv (model_from_rec, mpcb_model.h) and keeps the
// Model<T> in LDS (fp64: 24 values per group) or in each lane's registers (fp32), where rk4_nom of
// pass 1 and rk4_tan of passes 2 and 3 read it; the record joins the check sum.  PM = false is the
// kernel of mpcb_solve_iterate_pw unchanged.
//
// NaN rule (mpcb_eval's): every loaded input v adds v * 0 to a check sum, NaN unless v is finite;
// an instance whose sum is NaN gets status NAN and NaN in every output.  The groups of a wave
// share nothing but the barriers and the trip count of the active-set loop.
#include <hip/hip_runtime.h>

#include <limits>

#include "../../include/mpcb.h"
#include "mpcb_common.h"
#include "mpcb_pw.h"

namespace mpcb {
namespace {

constexpr int PW_SINK = 64;   // per slot: one element per lane

// an instance's weights in LDS, row-major as given
template <class T>
struct PwWeights {
  T Q[NX * NX];
  T R[NU * NU];
  T QN[NX * NX];
};

template <class T, int BOX, bool PM>
__global__ void __launch_bounds__(64) pw_kernel(PwArgs<T> a) {
  __shared__ GroupLds<T> lds_all[GROUPS];
  __shared__ PwWeights<T> w_all[GROUPS];
  // PM: the group's own vehicle, built in pass 1 from its record (uniform per 16-lane group, not per
  // wave, so it cannot sit in scalar registers); otherwise the handle's, a kernel argument.  fp64
  // keeps it in LDS (24 values per group; a copy per lane is 48 registers of a kernel that spills
  // already, measured: 220 B more scratch per lane).  fp32 has the registers, and every lane keeps
  // the copy it derives: the tangent's FMAs then read it without an LDS load each, which is the
  // whole cost of PM there
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
  PwWeights<T>& PW = w_all[q];
  const int N = a.N;
  constexpr int RN = Rec<BOX>::n;
  const T s = a.s;
  const Weights<T>& W = *a.W;
  T* slot = a.scratch + (int64_t)blockIdx.x * a.slot_elems;
  T* XU = slot;                                        // [(N+1)][64]         xbar | ubar
  T* CC = XU + (int64_t)(N + 1) * 64;                  // [N][GROUPS][CC_REC] lin. scalars | gap
  T* KR = CC + (int64_t)N * GROUPS * CC_REC;           // [N][64][RN]         gains (+box extras)
  T* sink = KR + (int64_t)N * 64 * RN;                 // [64]
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
    const T* xr = a.xref + b * a.xref_sb;
    const T* ur = a.uref + b * a.uref_sb;
    const T* x0p = a.x0 + b * a.x0_sb;
    const T* xbp = a.xbar + b * (int64_t)(N + 1) * NX;
    const T* ubp = a.ubar + b * (int64_t)N * NU;

    // ------------------------------------------------------------------ pass 1: nominal
    Model<T> Mi;   // PM: the instance's vehicle; every lane derives it (the record's 14 values join
                   // the check sum), and with PM_LDS lane 0 publishes it for the three passes
    if constexpr (PM) {
      model_from_rec<T>(a.model + b * a.model_sb, a.M.g, Mi, chk);
      if constexpr (PM_LDS) {
        if (j == 0) *Mg = Mi;
        __syncthreads();
      }
    }
    const Model<T>& M = PM_LDS ? *Mg : (PM ? Mi : a.M);
    {
      // the instance's weights: 144 + 16 + 144 values over the 16 lanes
      const T* Qp = a.Qw + b * a.Qw_sb;
      const T* Rp = a.Rw + b * a.Rw_sb;
      const T* QNp = a.QNw + b * a.QNw_sb;
#pragma unroll
      for (int i = 0; i < NX * NX / 16; ++i) {
        const T vq = Qp[i * 16 + j], vn = QNp[i * 16 + j];
        chk += vq * T(0) + vn * T(0);
        PW.Q[i * 16 + j] = vq;
        PW.QN[i * 16 + j] = vn;
      }
      const T vr = Rp[j];
      chk += vr * T(0) + x0p[jx] * T(0);
      PW.R[j] = vr;
    }
    for (int k = j; k < N; k += 16) {
      T xb[NX], ub[NU], xn[NX], nx[NX];
      load_vec<NX>(xbp + (int64_t)k * NX, xb);
      load_vec<NU>(ubp + (int64_t)k * NU, ub);
      load_vec<NX>(xbp + (int64_t)(k + 1) * NX, nx);
#pragma unroll
      for (int i = 0; i < NX; ++i) chk += xb[i] * T(0) + nx[i] * T(0) + xr[(int64_t)k * NX + i] * T(0);
#pragma unroll
      for (int m = 0; m < NU; ++m) chk += ub[m] * T(0) + ur[(int64_t)k * NU + m] * T(0);
      store_vec<NX>(XU + (int64_t)k * 64 + q * 16, xb);
      store_vec<NU>(XU + (int64_t)k * 64 + q * 16 + NX, ub);
      T* cc = CC + ((int64_t)k * GROUPS + q) * CC_REC;
      rk4_nom<T>(xb, ub, a.h, M, w, xn, [&](int stage, const T* c) { store_vec<LIN_N>(cc + stage * LIN_N, c); });
      T gp[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) gp[i] = xn[i] - nx[i];
      store_vec<NX>(cc + LIN_STAGE, gp);
    }
    if (j == 15) {   // the terminal stage, on the lane with the fewest stages
      T xb[NX];
      load_vec<NX>(xbp + (int64_t)N * NX, xb);
#pragma unroll
      for (int i = 0; i < NX; ++i) chk += xb[i] * T(0) + xr[(int64_t)N * NX + i] * T(0);
      store_vec<NX>(XU + (int64_t)N * 64 + q * 16, xb);
#pragma unroll
      for (int m = 0; m < NU; ++m) XU[(int64_t)N * 64 + q * 16 + NX + m] = T(0);
    }
    // every input has been read: the instance's check sum, the same in its 16 lanes
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) chk += __shfl_xor(chk, d, 16);
    const bool bad = chk != chk;
    __syncthreads();

    // the lane's column of blkdiag(Q, R) (the matrices are symmetric: column j = row j)
    T wcol[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) wcol[i] = j < NX ? PW.Q[i * NX + jx] : (i < NU ? PW.R[i * NU + ju] : T(0));

    uint64_t low[NU], up[NU];
#pragma unroll
    for (int m = 0; m < NU; ++m) { low[m] = 0; up[m] = 0; }
    bool done = false;
    bool qp_ok = true;
    int32_t st = MPCB_STATUS_OK;
    int best = 0x7fffffff, pcount = 3;   // Kim-Park safeguard state (uniform per group)

    for (int it = 0;; ++it) {
      // ------------------------------------------------------------------ pass 2: Riccati
      T pj;       // p_{k+1}[j]
      {
        const T xN = XU[(int64_t)N * 64 + q * 16 + jx];
        L.v[j] = (j < NX) ? xN - xr[(int64_t)N * NX + jx] : T(0);
        __syncthreads();
        T acc = T(0);
#pragma unroll
        for (int i = 0; i < NX; ++i) acc += PW.QN[i * NX + jx] * L.v[i];
        pj = acc;
        if (j < NX) {
#pragma unroll
          for (int i = 0; i < NX; ++i) L.P[j * NX + i] = PW.QN[i * NX + j];
        }
        __syncthreads();
      }
      bool pass_ok = true;
      for (int k = N - 1; k >= 0; --k) {
        T col[NX];
        const T* cc = CC + ((int64_t)k * GROUPS + q) * CC_REC;
        {
          // e = ybar - yref (component j), exchanged through LDS for block-diagonal W
          const T ybar = XU[(int64_t)k * 64 + lane];
          L.v[j] = ybar - ((j < NX) ? xr[(int64_t)k * NX + jx] : ur[(int64_t)k * NU + ju]);
          // tangent RK4 seeded with e_j: column j of [A|B]
          T dx[NX], du[NU];
#pragma unroll
          for (int i = 0; i < NX; ++i) dx[i] = (j == i) ? T(1) : T(0);
#pragma unroll
          for (int m = 0; m < NU; ++m) du[m] = (j == NX + m) ? T(1) : T(0);
          rk4_tan<T>(cc, dx, du, a.h, M, col);
          // gap b = Phi(xbar_k, ubar_k) - xbar_{k+1};  pt = p + P b  (P symmetric: row j = col j)
          T pt = pj;
#pragma unroll
          for (int i = 0; i < NX; ++i) pt += L.P[jx * NX + i] * cc[LIN_STAGE + i];
          L.hv[j] = pt;
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) L.X[j * NX + i] = col[i];
        __syncthreads();
        // h_j = col_j . pt
        T hj = T(0);
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
        {
          T acc = T(0);
          if (j < NX) {
#pragma unroll
            for (int i = 0; i < NX; ++i) {
              G[i] += s * wcol[i];
              acc += wcol[i] * L.v[i];
            }
          } else {
#pragma unroll
            for (int n = 0; n < NU; ++n) {
              G[NX + n] += s * wcol[n];
              acc += wcol[n] * L.v[NX + n];
            }
          }
          hj += s * acc;
        }
#pragma unroll
        for (int m = 0; m < NU; ++m) L.Hu[j * NU + m] = G[NX + m];
        __syncthreads();   // all reads of L.v / L.hv / L.X done; Hu visible
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
        // ---- input-box masking (fixed components: du_m = delta_m)
        if constexpr (BOX) {
          T ub[NU];
          load_vec<NU>(XU + (int64_t)k * 64 + q * 16 + NX, ub);
          bool fixed[NU];
          T delta[NU];
#pragma unroll
          for (int m = 0; m < NU; ++m) {
            const bool lo = (low[m] >> k) & 1ull, hi = (up[m] >> k) & 1ull;
            fixed[m] = lo || hi;
            delta[m] = lo ? (W.lbu[m] - ub[m]) : (hi ? (W.ubu[m] - ub[m]) : T(0));
          }
          T hn[NU];
#pragma unroll
          for (int m = 0; m < NU; ++m) {
            T acc = ht[m];
#pragma unroll
            for (int n = 0; n < NU; ++n) acc += fixed[n] ? Ht[m * NU + n] * delta[n] : T(0);
            hn[m] = fixed[m] ? -delta[m] : acc;
            Hux_t[m] = fixed[m] ? T(0) : Hux_t[m];
          }
#pragma unroll
          for (int m = 0; m < NU; ++m) {
            ht[m] = hn[m];
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
        pass_ok = pass_ok && ok;
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
        // ---- gains (and box extras): every lane stores RN values of its own record
        T* rec = KR + ((int64_t)k * 64 + lane) * RN;
        const T kf = sel<NU>(kff, ju);
#pragma unroll
        for (int m = 0; m < NU; ++m) rec[m] = j < NX ? Kj[m] : kf;
        if constexpr (BOX) {
          // input lanes: row NX+m of the stage Hessian (== this lane's column by symmetry) and
          // h_u[m]; the state lanes' copies are not read
#pragma unroll
          for (int i = 0; i < NZ; ++i) rec[4 + i] = G[i];
          rec[4 + NZ] = hj;
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
      if (!done) qp_ok = qp_ok && pass_ok;

      // ------------------------------------------------------------------ pass 3: forward
      // lanes NX+m: infeasibility sets of component m (bit k = stage k)
      uint64_t vlo = 0, vhi = 0, vfl = 0, vfu = 0;
      {
        // where this pass's stores go: lane j < NX owns X[.., j], lane NX + m owns U[.., m] and u0[m]
        const bool write = valid && !done;
        const bool outX = write && a.X && j < NX, outU = write && a.U && j >= NX, outu0 = write && j >= NX;
        T* const yp = outX ? a.X + b * (int64_t)(N + 1) * NX + jx
                           : (outU ? a.U + b * (int64_t)N * NU + ju : sink + lane);
        const int64_t ys = outX ? NX : (outU ? NU : 0);
        T* const u0p = outu0 ? a.u0 + b * NU + ju : sink + lane;
        T lbm = T(0), ubm = T(0);
        uint64_t lowm = 0, upm = 0;
        if constexpr (BOX) {
          lbm = W.lbu[ju];
          ubm = W.ubu[ju];
          lowm = sel<NU>(low, ju);
          upm = sel<NU>(up, ju);
        }
        T dxk[NX];
        {
          const T* p = XU + q * 16;
#pragma unroll
          for (int i = 0; i < NX; ++i) dxk[i] = x0p[i] - p[i];
        }
        for (int k = 0; k < N; ++k) {
          T duk[NU];
#pragma unroll
          for (int m = 0; m < NU; ++m) duk[m] = KR[((int64_t)k * 64 + q * 16 + NX + m) * RN];
#pragma unroll
          for (int l = 0; l < NX; ++l) {
            const T* r = KR + ((int64_t)k * 64 + q * 16 + l) * RN;
#pragma unroll
            for (int m = 0; m < NU; ++m) duk[m] += r[m] * dxk[l];
          }
          const T ybar = XU[(int64_t)k * 64 + lane];
          T val = ybar + (j < NX ? sel<NX>(dxk, jx) : sel<NU>(duk, ju));
          if constexpr (BOX) {
            if (j >= NX) {
              const T* r = KR + ((int64_t)k * 64 + lane) * RN;
              const bool lo = (lowm >> k) & 1ull, hi = (upm >> k) & 1ull;
              T mu = r[4 + NZ];
#pragma unroll
              for (int i = 0; i < NX; ++i) mu += r[4 + i] * dxk[i];
#pragma unroll
              for (int n = 0; n < NU; ++n) mu += r[4 + NX + n] * duk[n];
              const bool fr = !(lo || hi);
              vlo |= (uint64_t)(fr && val < lbm) << k;
              vhi |= (uint64_t)(fr && val > ubm) << k;
              vfl |= (uint64_t)(lo && mu < T(0)) << k;
              vfu |= (uint64_t)(hi && mu > T(0)) << k;
              // a clamped component is the bound's value itself
              val = lo ? lbm : (hi ? ubm : val);
            }
          }
          val = bad ? qnan : val;
          yp[k * ys] = val;
          if (k == 0) u0p[0] = val;
          const T* cc = CC + ((int64_t)k * GROUPS + q) * CC_REC;
          T dphi[NX];
          rk4_tan<T>(cc, dxk, duk, a.h, M, dphi);
#pragma unroll
          for (int i = 0; i < NX; ++i) dxk[i] = dphi[i] + cc[LIN_STAGE + i];
        }
        {
          const T xN = XU[(int64_t)N * 64 + q * 16 + jx];
          T* const xp = outX ? yp + (int64_t)N * NX : sink + lane;
          xp[0] = bad ? qnan : xN + sel<NX>(dxk, jx);
        }
      }

      if constexpr (!BOX) {
        break;
      } else {
        // active-set update (Kim-Park block principal pivoting, mirrors oracle.ocp.pdas_solve):
        // V = {free u<lb} U {free u>ub} U {at lb, mu<0} U {at ub, mu>0}; |V| = 0 <=> KKT.
        const uint64_t V = vlo | vhi | vfl | vfu;
        int cnt = (j >= NX) ? __popcll(V) : 0;
        int firstk = (j >= NX && V) ? __ffsll((long long)V) - 1 : 64;
        int nV = 0, first = 64 * NU;
#pragma unroll
        for (int m = 0; m < NU; ++m) {
          nV += __shfl(cnt, q * 16 + NX + m);
          const int fm = __shfl(firstk, q * 16 + NX + m) * NU + m;
          first = fm < first ? fm : first;
        }
        const bool gconv = nV == 0;
        const bool full = (nV < best) || (pcount > 0);
        pcount = (nV < best) ? 3 : (full ? pcount - 1 : pcount);
        best = nV < best ? nV : best;
        const uint64_t selm = full ? V : ((first < 64 * NU && (first % NU) == ju && j >= NX) ? (1ull << (first / NU)) : 0ull);
        const uint64_t nlow = (sel<NU>(low, ju) | (selm & vlo)) & ~(selm & vfl);
        const uint64_t nup = (sel<NU>(up, ju) | (selm & vhi)) & ~(selm & vfu);
#pragma unroll
        for (int m = 0; m < NU; ++m) {
          const int src = q * 16 + NX + m;
          const uint64_t nl = __shfl(nlow, src);
          const uint64_t nu_ = __shfl(nup, src);
          if (!done && !gconv) { low[m] = nl; up[m] = nu_; }
        }
        if (!done && gconv) done = true;
        const bool all_done = __all(done || !valid);
        if (all_done) break;
        if (it + 1 >= a.max_as_iter) {
          if (!done) st = MPCB_STATUS_MAXITER;
          break;
        }
      }
    }
    if (valid && j == 0)
      a.status[b] = bad ? MPCB_STATUS_NAN : (qp_ok ? st : MPCB_STATUS_QP_FAIL);
    __syncthreads();   // the next wave of the stride rewrites the slot and the LDS weights
  }
}

}  // namespace

int64_t pw_slot_elems(int N, int box) {
  const int RN = box ? Rec<1>::n : Rec<0>::n;
  return (int64_t)(N + 1) * 64 + (int64_t)N * GROUPS * CC_REC + (int64_t)N * 64 * RN + PW_SINK;
}

template <class T, bool PM> static hipError_t launch_pw_pm(const PwArgs<T>& a, int grid, hipStream_t st) {
  if constexpr (sizeof(T) == 8) {
    if (a.box) {
      hipLaunchKernelGGL((pw_kernel<T, 1, PM>), dim3(grid), dim3(64), 0, st, a);
      return hipGetLastError();
    }
  } else {
    if (a.box) return hipErrorInvalidValue;   // fp32 with the box is refused by the entry point
  }
  hipLaunchKernelGGL((pw_kernel<T, 0, PM>), dim3(grid), dim3(64), 0, st, a);
  return hipGetLastError();
}

// a.model == NULL: the instantiations of mpcb_solve_iterate_pw, whatever the caller
template <class T> hipError_t launch_pw(const PwArgs<T>& a, int grid, hipStream_t st) {
  return a.model ? launch_pw_pm<T, true>(a, grid, st) : launch_pw_pm<T, false>(a, grid, st);
}

template hipError_t launch_pw<double>(const PwArgs<double>&, int, hipStream_t);
template hipError_t launch_pw<float>(const PwArgs<float>&, int, hipStream_t);

}  // namespace mpcb
