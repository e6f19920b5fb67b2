// mpcb_gains.h — launch interface of the RTI step's feedback gains and cost-to-go Hessian for the
// 12/4 model (mpcb_gains.hip; mpcb_solve_gains in include/mpcb.h).  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpcb_kernels.h"

namespace mpcb {

template <class T>
struct GainsArgs {
  int64_t B;
  int N;
  int mask;                          // an active set is given: by `fixed`, or else read from U
  T h, s;                            // RK4 step, stage cost scaling
  Model<T> M;
  const Weights<T>* W;
  const T* xbar; const T* ubar;      // [B, N+1, nx], [B, N, nu]: the linearisation point
  const T* U;                        // [B, N, nu]: read only with mask and without fixed
  const uint8_t* fixed;              // [B, N, nu] nonzero = clamped, nullable
  const T* wind; int64_t wind_sb;    // nullable
  T* K; T* P0;                       // [B, N, nu, nx], [B, nx, nx], either nullable
  int32_t* status;
  T* scratch;                        // per-slot workspace (one slot = one wavefront = GROUPS instances)
  int64_t slot_elems;
  // mpcb_solve_gains_pm: instance b's vehicle record (MODEL_REC values) at model + b * model_sb;
  // NULL = the handle's M and the kernels of mpcb_solve_gains
  const T* model; int64_t model_sb;
};

// elements of one workspace slot: the captured linearisation scalars of N stages and the sinks of
// the stores of an output nobody asked for
int64_t gains_slot_elems(int N);
// grid: resident slots (the kernel strides over the waves of the batch)
template <class T> hipError_t launch_gains(const GainsArgs<T>& a, int grid, hipStream_t st);

}  // namespace mpcb
