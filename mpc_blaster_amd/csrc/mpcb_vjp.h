// mpcb_vjp.h — launch interface of the SQP_RTI step's vector-Jacobian product (mpcb_vjp.hip;
// mpcb_solve_vjp, mpcb_solve_vjp_w and mpcb_solve_vjp_pw in include/mpcb.h).  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpcb_kernels.h"

namespace mpcb {

template <class T>
struct VjpArgs {
  int64_t B;
  int N;
  int box;                           // input box on: the active set is read from U
  T h, s;                            // RK4 step, stage cost scaling
  Model<T> M;
  const Weights<T>* W;
  const T* xbar; const T* ubar;      // [B, N+1, nx], [B, N, nu]: the linearisation point
  const T* U;                        // [B, N, nu], nullable without the box
  const T* wind; int64_t wind_sb;    // nullable
  const T* gX; const T* gU;          // cotangents, either nullable
  T* gx0; T* gxref; T* guref;        // [B, nx], [B, N+1, nx], [B, N, nu], each nullable
  int32_t* status;
  T* scratch;                        // per-slot workspace (one slot = one wavefront = GROUPS instances)
  int64_t slot_elems;
  // weight gradients (mpcb_solve_vjp_w): any of gQ, gR, gQN non-null selects the kernel variant that
  // forms them, which reads the solve's output and its references (all four required then)
  const T* X;                        // [B, N+1, nx]; U above is then required without the box too
  const T* xref; int64_t xref_sb;    // the solve's references and per-instance strides (0 = broadcast)
  const T* uref; int64_t uref_sb;
  T* gQ; T* gR; T* gQN;              // [B, nx, nx], [B, nu, nu], [B, nx, nx], each nullable
  // per-instance weights (mpcb_solve_vjp_pw): Qw non-null selects the kernel variant that reads
  // instance b's matrices at Qw + b * Qw_sb and so on (all three set then; stride 0 = one for all)
  const T* Qw = nullptr; int64_t Qw_sb = 0;
  const T* Rw = nullptr; int64_t Rw_sb = 0;
  const T* QNw = nullptr; int64_t QNw_sb = 0;
};

// elements of one workspace slot: the captured linearisation scalars and the gains of N stages
int64_t vjp_slot_elems(int N);
// grid: resident slots (the kernel strides over the waves of the batch)
template <class T> hipError_t launch_vjp(const VjpArgs<T>& a, int grid, hipStream_t st);

}  // namespace mpcb
