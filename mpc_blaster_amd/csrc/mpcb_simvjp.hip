// mpcb_simvjp.hip — reverse mode of the plant step (mpcb_sim_step_vjp): with x_out = Phi_b(x, u) one
// RK4 step and gxn the cotangent of x_out, one sweep back through the four stages gives
// gx = (dPhi/dx)^T gxn, gu = (dPhi/du)^T gxn and, on request, the gradients with respect to the wind
// and to the vehicle record.  It is the exact derivative of the discrete RK4 map.
#include <hip/hip_runtime.h>

#include <limits>

#include "../../include/mpcb.h"
#include "mpcb_kernels.h"

namespace mpcb {

// One thread per instance, 256-thread blocks: the layout of sim_step_kernel.  The forward pass
// (rk4_nom) keeps the 4 x LIN_N captured scalars in registers, the backward pass (rk4_adj) consumes
// them last stage first.
//   PM: the vehicle is instance b's record (model_from_rec; its check sum joins the NaN rule),
//       otherwise the handle's Model<T> by value.
//   WM: gwind or gmodel is requested; the gx / gu-only instance carries no model accumulators.
// Every input is read before the first store, so gx may alias gxn (neither is __restrict__).
// No atomics: results are bit-reproducible.
template <class T, bool PM, bool WM>
__global__ void __launch_bounds__(256) sim_step_vjp_kernel(int64_t B, T h, Model<T> M0,
                                                           const T* __restrict__ model, int64_t model_sb,
                                                           const T* __restrict__ x,
                                                           const T* __restrict__ u,
                                                           const T* __restrict__ wind, int64_t wind_sb,
                                                           const T* gxn, T* gx, T* __restrict__ gu,
                                                           T* __restrict__ gwind, T* __restrict__ gmodel) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  Model<T> M;
  T chk = T(0);
  if constexpr (PM) model_from_rec<T>(model + b * model_sb, M0.g, M, chk);
  else M = M0;
  T w[3] = {T(0), T(0), T(0)};
  if (wind) { w[0] = wind[b * wind_sb]; w[1] = wind[b * wind_sb + 1]; w[2] = wind[b * wind_sb + 2]; }
  T xv[NX], uv[NU], lam[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) { xv[i] = x[b * NX + i]; lam[i] = gxn[b * NX + i]; }
#pragma unroll
  for (int m = 0; m < NU; ++m) uv[m] = u[b * NU + m];
#pragma unroll
  for (int i = 0; i < NX; ++i) chk += xv[i] * T(0) + lam[i] * T(0);
#pragma unroll
  for (int m = 0; m < NU; ++m) chk += uv[m] * T(0);
  chk += w[0] * T(0) + w[1] * T(0) + w[2] * T(0);

  T C[LIN_STAGE], xn[NX];
  rk4_nom<T>(xv, uv, h, M, w, xn, [&](int s, const T* c) {
#pragma unroll
    for (int i = 0; i < LIN_N; ++i) C[s * LIN_N + i] = c[i];
  });
  T px[NX], pu[NU];
  ModelAdj<T> G;
  if constexpr (WM) G.zero();
  rk4_adj<T, WM>(C, uv, h, M, w, lam, px, pu, G);

  const bool bad = chk != chk;
  const T nan = std::numeric_limits<T>::quiet_NaN();
  if (gx) {
#pragma unroll
    for (int i = 0; i < NX; ++i) gx[b * NX + i] = bad ? nan : px[i];
  }
  if (gu) {
#pragma unroll
    for (int m = 0; m < NU; ++m) gu[b * NU + m] = bad ? nan : pu[m];
  }
  if constexpr (WM) {
    if (gwind) {
#pragma unroll
      for (int i = 0; i < 3; ++i) gwind[b * 3 + i] = bad ? nan : G.w[i];
    }
    if (gmodel) {
      T r[MODEL_REC];
      model_adj_to_rec<T>(M, G, r);
#pragma unroll
      for (int i = 0; i < MODEL_REC; ++i) gmodel[b * MODEL_REC + i] = bad ? nan : r[i];
    }
  }
}

template <class T>
hipError_t launch_sim_step_vjp(int64_t B, T h, const Model<T>& M, const T* model, int64_t model_sb,
                               const T* x, const T* u, const T* wind, int64_t wind_sb, const T* gxn,
                               T* gx, T* gu, T* gwind, T* gmodel, hipStream_t st) {
  const dim3 grid((unsigned)((B + 255) / 256)), block(256);
  const bool wm = gwind || gmodel;
#define MPCB_SIMVJP(PM, WM)                                                                        \
  hipLaunchKernelGGL((sim_step_vjp_kernel<T, PM, WM>), grid, block, 0, st, B, h, M, model, model_sb, \
                     x, u, wind, wind_sb, gxn, gx, gu, gwind, gmodel)
  if (model) {
    if (wm) MPCB_SIMVJP(true, true); else MPCB_SIMVJP(true, false);
  } else {
    if (wm) MPCB_SIMVJP(false, true); else MPCB_SIMVJP(false, false);
  }
#undef MPCB_SIMVJP
  return hipGetLastError();
}

template hipError_t launch_sim_step_vjp<double>(int64_t, double, const Model<double>&, const double*, int64_t,
                                                const double*, const double*, const double*, int64_t,
                                                const double*, double*, double*, double*, double*, hipStream_t);
template hipError_t launch_sim_step_vjp<float>(int64_t, float, const Model<float>&, const float*, int64_t,
                                               const float*, const float*, const float*, int64_t, const float*,
                                               float*, float*, float*, float*, hipStream_t);

}  // namespace mpcb
