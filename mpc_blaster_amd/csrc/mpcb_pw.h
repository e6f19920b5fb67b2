// mpcb_pw.h — launch interface of the SQP_RTI step with per-instance cost weights for the 12/4 model
// (mpcb_pw.hip; mpcb_solve_iterate_pw in include/mpcb.h).  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpcb_kernels.h"

namespace mpcb {

template <class T>
struct PwArgs {
  int64_t B;
  int N;
  int box;                           // input box on (fp64 only): the primal-dual active set
  int max_as_iter;                   // ... and its cap in passes (no hand-over to an interior point)
  T h, s;                            // RK4 step, stage cost scaling
  Model<T> M;
  const Weights<T>* W;               // the handle's block: the input box
  const T* x0; int64_t x0_sb;
  const T* xref; int64_t xref_sb;
  const T* uref; int64_t uref_sb;
  const T* wind; int64_t wind_sb;    // nullable
  const T* xbar; const T* ubar;      // [B, N+1, nx], [B, N, nu]: the linearisation point
  // instance b's weights at Qw + b * Qw_sb (row-major, symmetric; stride 0 = one matrix for all);
  // never null here: the caller puts the handle's own matrix with stride 0 in place of NULL
  const T* Qw; int64_t Qw_sb;
  const T* Rw; int64_t Rw_sb;
  const T* QNw; int64_t QNw_sb;
  T* u0; T* X; T* U;                 // [B, nu], [B, N+1, nx], [B, N, nu]; X, U nullable, may alias xbar, ubar
  int32_t* status;
  T* scratch;                        // per-slot workspace (one slot = one wavefront = GROUPS instances)
  int64_t slot_elems;
  // mpcb_solve_iterate_pm: instance b's vehicle record (MODEL_REC values) at model + b * model_sb;
  // NULL = the handle's M and the kernels of mpcb_solve_iterate_pw
  const T* model; int64_t model_sb;
};

// elements of one workspace slot: the iterate, the captured linearisation scalars and gaps, the
// gains (with the box also the input rows of the stage Hessians) of N stages, and the store sink
int64_t pw_slot_elems(int N, int box);
// grid: resident slots (the kernel strides over the waves of the batch)
template <class T> hipError_t launch_pw(const PwArgs<T>& a, int grid, hipStream_t st);

}  // namespace mpcb
