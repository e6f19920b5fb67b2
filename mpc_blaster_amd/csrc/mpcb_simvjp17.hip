// mpcb_simvjp17.hip — reverse mode of the 17/6 plant step (mpcb_sim_step_vjp17): with
// x_out = Phi(x, u; p) one RK4 step of f17 and gxn the cotangent of x_out, one sweep back through the
// four stages gives gx = (dPhi/dx)^T gxn, gu = (dPhi/du)^T gxn and, on request, gparams =
// (dPhi/dp)^T gxn in the parameter vector's own column-major order.  It is the exact derivative of
// the discrete RK4 map.
#include <hip/hip_runtime.h>

#include <limits>

#include "../../include/mpcb.h"
#include "mpcb_full.h"

namespace mpcb {

// One thread per instance, 64-thread blocks: the layout of sim17_kernel.  The nominal pass
// (rk4_17_nom) keeps the 4 x F17_LIN_N captured scalars in registers, the sweep (rk4_17_adj)
// consumes them last stage first.
//   WP: gparams is requested.  The sweep then also accumulates d/dT_blast, and the 24 Jacobian
//       entries follow in closed form from the step's increment inc = x_out - x (nothing reads the
//       POC states, so the adjoint of poc_dot is gxn[14..16] times the RK4 weight at every stage):
//         gJp[i][c] = gxn[14+i] inc[c],  gJe[i][c] = gxn[14+i] inc[3+c],  gJa[i][c] = gxn[14+i] h u[4+c].
//       The gx / gu-only instance forms neither.
// Every input is read before the first store, so gx may alias gxn (neither is __restrict__).
// A non-finite x, u, gxn or parameter entry makes the check sum NaN and with it every requested row
// of that instance (x[0..2], x[14..16] and gxn[0] reach few or no outputs arithmetically).
// No atomics: results are bit-reproducible.
template <class T, bool WP>
__global__ void __launch_bounds__(64) sim_step_vjp17_kernel(int64_t B, T h, Model<T> M,
                                                            const T* __restrict__ p, int64_t p_sb,
                                                            const T* __restrict__ x,
                                                            const T* __restrict__ u, const T* gxn,
                                                            T* gx, T* __restrict__ gu,
                                                            T* __restrict__ gparams) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const T* pb = p + b * p_sb;
  P17<T> P;
  unpack_p17(pb, P);
  T xv[NX17], uv[NU17], lam[NX17];
#pragma unroll
  for (int i = 0; i < NX17; ++i) { xv[i] = x[b * NX17 + i]; lam[i] = gxn[b * NX17 + i]; }
#pragma unroll
  for (int m = 0; m < NU17; ++m) uv[m] = u[b * NU17 + m];
  T chk = T(0);
#pragma unroll
  for (int i = 0; i < NX17; ++i) chk += xv[i] * T(0) + lam[i] * T(0);
#pragma unroll
  for (int m = 0; m < NU17; ++m) chk += uv[m] * T(0);
#pragma unroll
  for (int i = 0; i < NP17; ++i) chk += pb[i] * T(0);

  T C[F17_LIN_STAGE], inc[NX17];
  rk4_17_nom<T>(xv, uv, h, M, P, inc, C);
  T px[NX17], pu[NU17], gtb = T(0);
  rk4_17_adj<T, WP>(C, uv, h, M, P, lam, px, pu, gtb);

  const bool bad = chk != chk;
  const T nan = std::numeric_limits<T>::quiet_NaN();
  if (gx) {
#pragma unroll
    for (int i = 0; i < NX17; ++i) gx[b * NX17 + i] = bad ? nan : px[i];
  }
  if (gu) {
#pragma unroll
    for (int m = 0; m < NU17; ++m) gu[b * NU17 + m] = bad ? nan : pu[m];
  }
  if constexpr (WP) {
    T* g = gparams + b * NP17;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const T q = lam[14 + i];
#pragma unroll
      for (int j = 0; j < 2; ++j) g[j * 3 + i] = bad ? nan : q * (h * uv[4 + j]);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        g[6 + j * 3 + i] = bad ? nan : q * inc[3 + j];
        g[15 + j * 3 + i] = bad ? nan : q * inc[j];
      }
    }
    g[24] = bad ? nan : gtb;
  }
}

template <class T>
hipError_t launch_sim_step_vjp17(int64_t B, T h, const Model<T>& M, const T* p, int64_t p_sb, const T* x,
                                 const T* u, const T* gxn, T* gx, T* gu, T* gparams, hipStream_t st) {
  const dim3 grid((unsigned)((B + 63) / 64)), block(64);
  if (gparams)
    hipLaunchKernelGGL((sim_step_vjp17_kernel<T, true>), grid, block, 0, st, B, h, M, p, p_sb, x, u, gxn, gx,
                       gu, gparams);
  else
    hipLaunchKernelGGL((sim_step_vjp17_kernel<T, false>), grid, block, 0, st, B, h, M, p, p_sb, x, u, gxn, gx,
                       gu, gparams);
  return hipGetLastError();
}

template hipError_t launch_sim_step_vjp17<double>(int64_t, double, const Model<double>&, const double*, int64_t,
                                                  const double*, const double*, const double*, double*, double*,
                                                  double*, hipStream_t);
template hipError_t launch_sim_step_vjp17<float>(int64_t, float, const Model<float>&, const float*, int64_t,
                                                 const float*, const float*, const float*, float*, float*, float*,
                                                 hipStream_t);

}  // namespace mpcb
