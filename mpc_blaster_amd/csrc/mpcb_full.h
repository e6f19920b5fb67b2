// mpcb_full.h — the full 17-state / 6-input BLASTER model on the device.
//
// Restates f_expl_expr of src/scripts/blastermodel.py:70-201 with every state and parameter:
//   x = [p(3), eta = (phi, theta, psi), v(3), omega(3), alpha(2), poc(3)]      (:171-190)
//   u = [T0..T3, alpha1_dot, alpha2_dot]                                       (:191-193)
//   p = vec(J_angles 3x2) | vec(J_euler 3x3) | vec(J_p 3x3) | T_blast (column-major, :203-210)
//   p_dot     = v
//   eta_dot   = inv(R_to_omega(phi, theta)) omega                              (:128-141, :162)
//   v_dot     = R (e3 sum T + R_gimbal e3 T_blast) / m - g e3                   (:143-163)
//               R = Rz Ry Rx (:103-122), R_gimbal e3 = Ry(a1) Rx(a2) e3 = [s1 c2, -s2, c1 c2]
//   omega_dot = inv(J) (M(T) - omega x J omega)                                (:95-101, :164)
//   alpha_dot = u[4:6]
//   poc_dot   = J_p v + J_euler eta_dot + J_angles alpha_dot                   (:165-167)
// ``f17_tan`` evaluates f and one directional derivative J_f (dx, du) in the same pass
// (forward-mode dual numbers: each lane of an instance seeds one of the 23 directions).
#pragma once
#include <hip/hip_runtime.h>

#include "mpcb_common.h"
#include "mpcb_model.h"

namespace mpcb {

constexpr int NX17 = 17, NU17 = 6, NZ17 = NX17 + NU17, NP17 = 25;

// per-instance parameters unpacked from the 25-vector (row-major blocks)
template <class T>
struct P17 {
  T Ja[6];   // J_angles 3x2
  T Je[9];   // J_euler  3x3
  T Jp[9];   // J_p      3x3
  T tb;      // T_blast
};

template <class T>
__device__ __forceinline__ void unpack_p17(const T* __restrict__ p, P17<T>& P) {
  // column-major vec (blastermodel.py:203-210): block[i][j] = p[off + j*3 + i]
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) P.Ja[i * 2 + j] = p[j * 3 + i];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      P.Je[i * 3 + j] = p[6 + j * 3 + i];
      P.Jp[i * 3 + j] = p[15 + j * 3 + i];
    }
  }
  P.tb = p[24];
}

// sin/cos of the five angles of f17 (Euler angles x[3..5], swivel angles x[12..13]), one thread
struct Trig17Serial {
  template <class T>
  __device__ __forceinline__ void operator()(const T* __restrict__ x, T (&s)[5], T (&c)[5]) const {
    sc(x[3], &s[0], &c[0]);
    sc(x[4], &s[1], &c[1]);
    sc(x[5], &s[2], &c[2]);
    sc(x[12], &s[3], &c[3]);
    sc(x[13], &s[4], &c[4]);
  }
};

template <class T, bool TAN, class Trig = Trig17Serial>
__device__ __forceinline__ void f17_tan(const T* __restrict__ x, const T* __restrict__ dx,
                                        const T* __restrict__ u, const T* __restrict__ du,
                                        const Model<T>& M, const P17<T>& P, T* __restrict__ f,
                                        T* __restrict__ df, const Trig& trig = Trig()) {
  T tsn[5], tcs[5];
  trig(x, tsn, tcs);
  const T sf = tsn[0], cf = tcs[0], st = tsn[1], ct = tcs[1], sp = tsn[2], cp = tcs[2];
  const T s1 = tsn[3], c1 = tcs[3], s2 = tsn[4], c2 = tcs[4];
  const T ict = recip(ct);
  const T tt = st * ict;
  const T wx = x[9], wy = x[10], wz = x[11];
  f[0] = x[6]; f[1] = x[7]; f[2] = x[8];
  const T a = sf * wy + cf * wz;
  const T b = cf * wy - sf * wz;
  const T ed0 = wx + tt * a, ed1 = b, ed2 = a * ict;
  f[3] = ed0; f[4] = ed1; f[5] = ed2;
  // R = Rz(psi) Ry(theta) Rx(phi)
  const T cpst = cp * st, spst = sp * st;
  const T R00 = cp * ct, R01 = cpst * sf - sp * cf, R02 = cpst * cf + sp * sf;
  const T R10 = sp * ct, R11 = spst * sf + cp * cf, R12 = spst * cf - cp * sf;
  const T R20 = -st, R21 = ct * sf, R22 = ct * cf;
  // body force: motors along e3 plus the swivelled blaster thrust
  const T Tsum = (u[0] + u[1]) + (u[2] + u[3]);
  const T fb0 = P.tb * (s1 * c2), fb1 = -P.tb * s2, fb2 = Tsum + P.tb * (c1 * c2);
  f[6] = (R00 * fb0 + R01 * fb1 + R02 * fb2) * M.minv;
  f[7] = (R10 * fb0 + R11 * fb1 + R12 * fb2) * M.minv;
  f[8] = (R20 * fb0 + R21 * fb1 + R22 * fb2) * M.minv - M.g;
  const T jw0 = M.J[0] * wx + M.J[1] * wy + M.J[2] * wz;
  const T jw1 = M.J[3] * wx + M.J[4] * wy + M.J[5] * wz;
  const T jw2 = M.J[6] * wx + M.J[7] * wy + M.J[8] * wz;
  const T k0 = wy * jw2 - wz * jw1;
  const T k1 = wz * jw0 - wx * jw2;
  const T k2 = wx * jw1 - wy * jw0;
  const T m0 = (u[1] + u[3] - u[0] - u[2]) * M.ly - k0;
  const T m1 = (u[1] + u[2] - u[0] - u[3]) * M.lx - k1;
  const T m2 = (u[2] + u[3] - u[0] - u[1]) * M.c - k2;
  f[9] = M.Jinv[0] * m0 + M.Jinv[1] * m1 + M.Jinv[2] * m2;
  f[10] = M.Jinv[3] * m0 + M.Jinv[4] * m1 + M.Jinv[5] * m2;
  f[11] = M.Jinv[6] * m0 + M.Jinv[7] * m1 + M.Jinv[8] * m2;
  f[12] = u[4];
  f[13] = u[5];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    f[14 + i] = P.Jp[i * 3] * x[6] + P.Jp[i * 3 + 1] * x[7] + P.Jp[i * 3 + 2] * x[8] +
                P.Je[i * 3] * ed0 + P.Je[i * 3 + 1] * ed1 + P.Je[i * 3 + 2] * ed2 +
                P.Ja[i * 2] * u[4] + P.Ja[i * 2 + 1] * u[5];
  if constexpr (TAN) {
    const T dphi = dx[3], dth = dx[4], dpsi = dx[5];
    const T dwx = dx[9], dwy = dx[10], dwz = dx[11];
    const T dsf = cf * dphi, dcf = -sf * dphi;
    const T dst = ct * dth, dct = -st * dth;
    const T dsp = cp * dpsi, dcp = -sp * dpsi;
    const T ds1 = c1 * dx[12], dc1 = -s1 * dx[12];
    const T ds2 = c2 * dx[13], dc2 = -s2 * dx[13];
    const T dict = -ict * ict * dct;
    const T dtt = dst * ict + st * dict;
    df[0] = dx[6]; df[1] = dx[7]; df[2] = dx[8];
    const T da = dsf * wy + sf * dwy + dcf * wz + cf * dwz;
    const T db = dcf * wy + cf * dwy - dsf * wz - sf * dwz;
    const T ded0 = dwx + dtt * a + tt * da, ded1 = db, ded2 = da * ict + a * dict;
    df[3] = ded0; df[4] = ded1; df[5] = ded2;
    const T dcpst = dcp * st + cp * dst, dspst = dsp * st + sp * dst;
    const T dR00 = dcp * ct + cp * dct;
    const T dR01 = dcpst * sf + cpst * dsf - dsp * cf - sp * dcf;
    const T dR02 = dcpst * cf + cpst * dcf + dsp * sf + sp * dsf;
    const T dR10 = dsp * ct + sp * dct;
    const T dR11 = dspst * sf + spst * dsf + dcp * cf + cp * dcf;
    const T dR12 = dspst * cf + spst * dcf - dcp * sf - cp * dsf;
    const T dR20 = -dst, dR21 = dct * sf + ct * dsf, dR22 = dct * cf + ct * dcf;
    const T dTsum = (du[0] + du[1]) + (du[2] + du[3]);
    const T dfb0 = P.tb * (ds1 * c2 + s1 * dc2), dfb1 = -P.tb * ds2;
    const T dfb2 = dTsum + P.tb * (dc1 * c2 + c1 * dc2);
    df[6] = (dR00 * fb0 + dR01 * fb1 + dR02 * fb2 + R00 * dfb0 + R01 * dfb1 + R02 * dfb2) * M.minv;
    df[7] = (dR10 * fb0 + dR11 * fb1 + dR12 * fb2 + R10 * dfb0 + R11 * dfb1 + R12 * dfb2) * M.minv;
    df[8] = (dR20 * fb0 + dR21 * fb1 + dR22 * fb2 + R20 * dfb0 + R21 * dfb1 + R22 * dfb2) * M.minv;
    const T djw0 = M.J[0] * dwx + M.J[1] * dwy + M.J[2] * dwz;
    const T djw1 = M.J[3] * dwx + M.J[4] * dwy + M.J[5] * dwz;
    const T djw2 = M.J[6] * dwx + M.J[7] * dwy + M.J[8] * dwz;
    const T dk0 = dwy * jw2 + wy * djw2 - dwz * jw1 - wz * djw1;
    const T dk1 = dwz * jw0 + wz * djw0 - dwx * jw2 - wx * djw2;
    const T dk2 = dwx * jw1 + wx * djw1 - dwy * jw0 - wy * djw0;
    const T dm0 = (du[1] + du[3] - du[0] - du[2]) * M.ly - dk0;
    const T dm1 = (du[1] + du[2] - du[0] - du[3]) * M.lx - dk1;
    const T dm2 = (du[2] + du[3] - du[0] - du[1]) * M.c - dk2;
    df[9] = M.Jinv[0] * dm0 + M.Jinv[1] * dm1 + M.Jinv[2] * dm2;
    df[10] = M.Jinv[3] * dm0 + M.Jinv[4] * dm1 + M.Jinv[5] * dm2;
    df[11] = M.Jinv[6] * dm0 + M.Jinv[7] * dm1 + M.Jinv[8] * dm2;
    df[12] = du[4];
    df[13] = du[5];
#pragma unroll
    for (int i = 0; i < 3; ++i)
      df[14 + i] = P.Jp[i * 3] * dx[6] + P.Jp[i * 3 + 1] * dx[7] + P.Jp[i * 3 + 2] * dx[8] +
                   P.Je[i * 3] * ded0 + P.Je[i * 3 + 1] * ded1 + P.Je[i * 3 + 2] * ded2 +
                   P.Ja[i * 2] * du[4] + P.Ja[i * 2 + 1] * du[5];
  }
}

// One classic RK4 step (acados sim_erk: 4 stages, 1 step) of f17 with an optional tangent.
template <class T, bool TAN, class Trig = Trig17Serial>
__device__ __forceinline__ void rk4_17(const T* __restrict__ x, const T* __restrict__ dx,
                                       const T* __restrict__ u, const T* __restrict__ du, T h,
                                       const Model<T>& M, const P17<T>& P, T* __restrict__ xn,
                                       T* __restrict__ dxn, const Trig& trig = Trig()) {
  T k[NX17], dk[NX17], xs[NX17], dxs[NX17];
  const T h2 = T(0.5) * h, h6 = h / T(6);
  f17_tan<T, TAN>(x, dx, u, du, M, P, k, dk, trig);
#pragma unroll
  for (int i = 0; i < NX17; ++i) {
    xn[i] = k[i];
    xs[i] = x[i] + h2 * k[i];
    if constexpr (TAN) { dxn[i] = dk[i]; dxs[i] = dx[i] + h2 * dk[i]; }
  }
  f17_tan<T, TAN>(xs, dxs, u, du, M, P, k, dk, trig);
#pragma unroll
  for (int i = 0; i < NX17; ++i) {
    xn[i] += T(2) * k[i];
    xs[i] = x[i] + h2 * k[i];
    if constexpr (TAN) { dxn[i] += T(2) * dk[i]; dxs[i] = dx[i] + h2 * dk[i]; }
  }
  f17_tan<T, TAN>(xs, dxs, u, du, M, P, k, dk, trig);
#pragma unroll
  for (int i = 0; i < NX17; ++i) {
    xn[i] += T(2) * k[i];
    xs[i] = x[i] + h * k[i];
    if constexpr (TAN) { dxn[i] += T(2) * dk[i]; dxs[i] = dx[i] + h * dk[i]; }
  }
  f17_tan<T, TAN>(xs, dxs, u, du, M, P, k, dk, trig);
#pragma unroll
  for (int i = 0; i < NX17; ++i) {
    xn[i] = x[i] + h6 * (xn[i] + k[i]);
    if constexpr (TAN) dxn[i] = dx[i] + h6 * (dxn[i] + dk[i]);
  }
}

// ---------------------------------------------------------------------------------------------
// Reverse mode of rk4_17 (mpcb_sim_step_vjp17): the 17/6 counterpart of f_nom_lin / f_adj_lin /
// rk4_adj in mpcb_model.h.  The nominal pass captures F17_LIN_N scalars per RK4 stage, the sweep
// applies the transpose of f17_tan's TAN branch from them: no transcendental, no division.
// ---------------------------------------------------------------------------------------------
constexpr int F17_LIN_N = 15;      // captured scalars per RK4 stage
constexpr int F17_LIN_STAGE = 60;  // per step (4 stages)

// f17 (the expressions of f17_tan) and the stage's captured scalars
//   c = [sf cf st ct sp cp s1 c1 s2 c2 | ict A | wx wy wz],  A = sf wy + cf wz.
// What else the sweep needs (tt, R, the body force, J w) it recomputes from these by products.
template <class T>
__device__ __forceinline__ void f17_nom_lin(const T* __restrict__ x, const T* __restrict__ u,
                                            const Model<T>& M, const P17<T>& P, T* __restrict__ f,
                                            T* __restrict__ c) {
  T tsn[5], tcs[5];
  Trig17Serial()(x, tsn, tcs);
  const T sf = tsn[0], cf = tcs[0], st = tsn[1], ct = tcs[1], sp = tsn[2], cp = tcs[2];
  const T s1 = tsn[3], c1 = tcs[3], s2 = tsn[4], c2 = tcs[4];
  const T ict = recip(ct);
  const T tt = st * ict;
  const T wx = x[9], wy = x[10], wz = x[11];
  f[0] = x[6]; f[1] = x[7]; f[2] = x[8];
  const T a = sf * wy + cf * wz;
  const T b = cf * wy - sf * wz;
  const T ed0 = wx + tt * a, ed1 = b, ed2 = a * ict;
  f[3] = ed0; f[4] = ed1; f[5] = ed2;
  const T cpst = cp * st, spst = sp * st;
  const T R00 = cp * ct, R01 = cpst * sf - sp * cf, R02 = cpst * cf + sp * sf;
  const T R10 = sp * ct, R11 = spst * sf + cp * cf, R12 = spst * cf - cp * sf;
  const T R20 = -st, R21 = ct * sf, R22 = ct * cf;
  const T Tsum = (u[0] + u[1]) + (u[2] + u[3]);
  const T fb0 = P.tb * (s1 * c2), fb1 = -P.tb * s2, fb2 = Tsum + P.tb * (c1 * c2);
  f[6] = (R00 * fb0 + R01 * fb1 + R02 * fb2) * M.minv;
  f[7] = (R10 * fb0 + R11 * fb1 + R12 * fb2) * M.minv;
  f[8] = (R20 * fb0 + R21 * fb1 + R22 * fb2) * M.minv - M.g;
  const T jw0 = M.J[0] * wx + M.J[1] * wy + M.J[2] * wz;
  const T jw1 = M.J[3] * wx + M.J[4] * wy + M.J[5] * wz;
  const T jw2 = M.J[6] * wx + M.J[7] * wy + M.J[8] * wz;
  const T m0 = (u[1] + u[3] - u[0] - u[2]) * M.ly - (wy * jw2 - wz * jw1);
  const T m1 = (u[1] + u[2] - u[0] - u[3]) * M.lx - (wz * jw0 - wx * jw2);
  const T m2 = (u[2] + u[3] - u[0] - u[1]) * M.c - (wx * jw1 - wy * jw0);
  f[9] = M.Jinv[0] * m0 + M.Jinv[1] * m1 + M.Jinv[2] * m2;
  f[10] = M.Jinv[3] * m0 + M.Jinv[4] * m1 + M.Jinv[5] * m2;
  f[11] = M.Jinv[6] * m0 + M.Jinv[7] * m1 + M.Jinv[8] * m2;
  f[12] = u[4];
  f[13] = u[5];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    f[14 + i] = P.Jp[i * 3] * x[6] + P.Jp[i * 3 + 1] * x[7] + P.Jp[i * 3 + 2] * x[8] +
                P.Je[i * 3] * ed0 + P.Je[i * 3 + 1] * ed1 + P.Je[i * 3 + 2] * ed2 +
                P.Ja[i * 2] * u[4] + P.Ja[i * 2 + 1] * u[5];
  c[0] = sf; c[1] = cf; c[2] = st; c[3] = ct; c[4] = sp; c[5] = cp;
  c[6] = s1; c[7] = c1; c[8] = s2; c[9] = c2; c[10] = ict; c[11] = a;
  c[12] = wx; c[13] = wy; c[14] = wz;
}

// px += (df/dx)^T a, pu += (df/du)^T a and, with WP, gtb += (df/dT_blast)^T a at the stage whose
// scalars are c: the transpose of f17_tan's TAN branch.  Relative to f_adj_lin (mpcb_model.h):
//  * the POC rows q = a[14..16] reach v (J_p^T q), the Euler rates (J_e^T q joins their adjoint
//    before the Euler-rate block) and the swivel rates (J_a^T q);
//  * v_dot = minv R fb with the full rotation and fb = (tb s1 c2, -tb s2, Tsum + tb c1 c2):
//    gfb = minv R^T a[6..8] feeds the swivel angles, the motors and T_blast, gR = minv a[6..8] fb^T
//    the six attitude trig adjoints.
// Nothing reads the POC states, so px[14..16] is left alone.  The 24 Jacobian entries of the
// parameter gradient have a closed form outside the sweep (rk4_17_adj).
template <class T, bool WP>
__device__ __forceinline__ void f17_adj_lin(const T* __restrict__ c, const T* __restrict__ u,
                                            const Model<T>& M, const P17<T>& P, const T* __restrict__ a,
                                            T* __restrict__ px, T* __restrict__ pu, T& gtb) {
  const T sf = c[0], cf = c[1], st = c[2], ct = c[3], sp = c[4], cp = c[5];
  const T s1 = c[6], c1 = c[7], s2 = c[8], c2 = c[9], ict = c[10], av = c[11];
  const T wx = c[12], wy = c[13], wz = c[14];
  const T tt = st * ict;
  const T q0 = a[14], q1 = a[15], q2 = a[16];
  // ---- p_dot = v, and J_p v in the POC rows
  px[6] += a[0] + (P.Jp[0] * q0 + P.Jp[3] * q1 + P.Jp[6] * q2);
  px[7] += a[1] + (P.Jp[1] * q0 + P.Jp[4] * q1 + P.Jp[7] * q2);
  px[8] += a[2] + (P.Jp[2] * q0 + P.Jp[5] * q1 + P.Jp[8] * q2);
  // ---- alpha_dot = u[4..5], and J_a alpha_dot in the POC rows
  pu[4] += a[12] + (P.Ja[0] * q0 + P.Ja[2] * q1 + P.Ja[4] * q2);
  pu[5] += a[13] + (P.Ja[1] * q0 + P.Ja[3] * q1 + P.Ja[5] * q2);
  // ---- eta_dot: ed0 = wx + tt A, ed1 = b, ed2 = A ict, read by f[3..5] and by J_e eta_dot
  const T e0 = a[3] + (P.Je[0] * q0 + P.Je[3] * q1 + P.Je[6] * q2);
  const T e1 = a[4] + (P.Je[1] * q0 + P.Je[4] * q1 + P.Je[7] * q2);
  const T e2 = a[5] + (P.Je[2] * q0 + P.Je[5] * q1 + P.Je[8] * q2);
  const T gA = tt * e0 + ict * e2;
  const T gtt = av * e0;
  const T gict = av * e2 + st * gtt;
  T gst = ict * gtt;
  T gct = -(ict * ict) * gict;
  T gsf = wy * gA - wz * e1;
  T gcf = wz * gA + wy * e1;
  T gwx = e0;
  T gwy = sf * gA + cf * e1;
  T gwz = cf * gA - sf * e1;
  // ---- v_dot = minv R fb - g e3
  const T cpst = cp * st, spst = sp * st;
  const T R00 = cp * ct, R01 = cpst * sf - sp * cf, R02 = cpst * cf + sp * sf;
  const T R10 = sp * ct, R11 = spst * sf + cp * cf, R12 = spst * cf - cp * sf;
  const T R20 = -st, R21 = ct * sf, R22 = ct * cf;
  const T Tsum = (u[0] + u[1]) + (u[2] + u[3]);
  const T s1c2 = s1 * c2, c1c2 = c1 * c2;
  const T fb0 = P.tb * s1c2, fb1 = -P.tb * s2, fb2 = Tsum + P.tb * c1c2;
  const T v0 = M.minv * a[6], v1 = M.minv * a[7], v2 = M.minv * a[8];
  const T gfb0 = R00 * v0 + R10 * v1 + R20 * v2;
  const T gfb1 = R01 * v0 + R11 * v1 + R21 * v2;
  const T gfb2 = R02 * v0 + R12 * v1 + R22 * v2;
  // gR[r][c] = v_r fb_c into the trig adjoints
  const T g01 = v0 * fb1, g02 = v0 * fb2, g11 = v1 * fb1, g12 = v1 * fb2;
  const T gcpst = sf * g01 + cf * g02;
  const T gspst = sf * g11 + cf * g12;
  T gcp = ct * (v0 * fb0) + cf * g11 - sf * g12 + st * gcpst;
  T gsp = ct * (v1 * fb0) - cf * g01 + sf * g02 + st * gspst;
  gct += cp * (v0 * fb0) + sp * (v1 * fb0) + sf * (v2 * fb1) + cf * (v2 * fb2);
  gst += cp * gcpst + sp * gspst - v2 * fb0;
  gsf += cpst * g01 + sp * g02 + spst * g11 - cp * g12 + ct * (v2 * fb1);
  gcf += cpst * g02 - sp * g01 + cp * g11 + spst * g12 + ct * (v2 * fb2);
  px[3] += cf * gsf - sf * gcf;
  px[4] += ct * gst - st * gct;
  px[5] += cp * gsp - sp * gcp;
  // the swivelled thrust: fb = (tb s1 c2, -tb s2, Tsum + tb c1 c2)
  const T gs1 = P.tb * c2 * gfb0, gc1 = P.tb * c2 * gfb2;
  const T gs2 = -P.tb * gfb1, gc2 = P.tb * (s1 * gfb0 + c1 * gfb2);
  px[12] += c1 * gs1 - s1 * gc1;
  px[13] += c2 * gs2 - s2 * gc2;
  if constexpr (WP) gtb += s1c2 * gfb0 - s2 * gfb1 + c1c2 * gfb2;
  // ---- omega_dot = Jinv m,  m = Mom(u) - w x J w
  const T gm0 = M.Jinv[0] * a[9] + M.Jinv[3] * a[10] + M.Jinv[6] * a[11];
  const T gm1 = M.Jinv[1] * a[9] + M.Jinv[4] * a[10] + M.Jinv[7] * a[11];
  const T gm2 = M.Jinv[2] * a[9] + M.Jinv[5] * a[10] + M.Jinv[8] * a[11];
  const T m0 = M.ly * gm0, m1 = M.lx * gm1, m2 = M.c * gm2;
  pu[0] += gfb2 - m0 - m1 - m2;
  pu[1] += gfb2 + m0 + m1 - m2;
  pu[2] += gfb2 - m0 + m1 + m2;
  pu[3] += gfb2 + m0 - m1 + m2;
  const T jw0 = M.J[0] * wx + M.J[1] * wy + M.J[2] * wz;
  const T jw1 = M.J[3] * wx + M.J[4] * wy + M.J[5] * wz;
  const T jw2 = M.J[6] * wx + M.J[7] * wy + M.J[8] * wz;
  gwx += jw2 * gm1 - jw1 * gm2;
  gwy += jw0 * gm2 - jw2 * gm0;
  gwz += jw1 * gm0 - jw0 * gm1;
  const T gj0 = wy * gm2 - wz * gm1;
  const T gj1 = wz * gm0 - wx * gm2;
  const T gj2 = wx * gm1 - wy * gm0;
  px[9] += gwx + M.J[0] * gj0 + M.J[3] * gj1 + M.J[6] * gj2;
  px[10] += gwy + M.J[1] * gj0 + M.J[4] * gj1 + M.J[7] * gj2;
  px[11] += gwz + M.J[2] * gj0 + M.J[5] * gj1 + M.J[8] * gj2;
}

// Nominal RK4 step of f17 that keeps every stage's captured scalars in C (F17_LIN_STAGE values,
// stage-major) and returns the step's increment inc = x_out - x = h/6 (k1 + 2 k2 + 2 k3 + k4),
// formed without the subtraction.
template <class T>
__device__ __forceinline__ void rk4_17_nom(const T* __restrict__ x, const T* __restrict__ u, T h,
                                           const Model<T>& M, const P17<T>& P, T* __restrict__ inc,
                                           T* __restrict__ C) {
  T k[NX17], xs[NX17];
  const T h2 = T(0.5) * h, h6 = h / T(6);
  f17_nom_lin<T>(x, u, M, P, k, C);
#pragma unroll
  for (int i = 0; i < NX17; ++i) { inc[i] = k[i]; xs[i] = x[i] + h2 * k[i]; }
  f17_nom_lin<T>(xs, u, M, P, k, C + F17_LIN_N);
#pragma unroll
  for (int i = 0; i < NX17; ++i) { inc[i] += T(2) * k[i]; xs[i] = x[i] + h2 * k[i]; }
  f17_nom_lin<T>(xs, u, M, P, k, C + 2 * F17_LIN_N);
#pragma unroll
  for (int i = 0; i < NX17; ++i) { inc[i] += T(2) * k[i]; xs[i] = x[i] + h * k[i]; }
  f17_nom_lin<T>(xs, u, M, P, k, C + 3 * F17_LIN_N);
#pragma unroll
  for (int i = 0; i < NX17; ++i) inc[i] = h6 * (inc[i] + k[i]);
}

// Reverse sweep of rk4_17_nom by the recurrence documented at rk4_adj (mpcb_model.h): lam is the
// cotangent of x_out, gx = (dPhi/dx)^T lam, gu = (dPhi/du)^T lam, gtb = (dPhi/dT_blast)^T lam (WP).
// px[14..16] stays 0 at every stage, so a[14 + i] is lam[14 + i] times the stage's RK4 weight.
template <class T, bool WP>
__device__ __forceinline__ void rk4_17_adj(const T* __restrict__ C, const T* __restrict__ u, T h,
                                           const Model<T>& M, const P17<T>& P, const T* __restrict__ lam,
                                           T* __restrict__ gx, T* __restrict__ gu, T& gtb) {
  const T h2 = T(0.5) * h, h6 = h / T(6), h3 = h / T(3);
  T a[NX17], p[NX17];
#pragma unroll
  for (int m = 0; m < NU17; ++m) gu[m] = T(0);
#pragma unroll
  for (int i = 0; i < NX17; ++i) { gx[i] = lam[i]; a[i] = h6 * lam[i]; p[i] = T(0); }
  f17_adj_lin<T, WP>(C + 3 * F17_LIN_N, u, M, P, a, p, gu, gtb);
#pragma unroll
  for (int i = 0; i < NX17; ++i) { gx[i] += p[i]; a[i] = h3 * lam[i] + h * p[i]; p[i] = T(0); }
  f17_adj_lin<T, WP>(C + 2 * F17_LIN_N, u, M, P, a, p, gu, gtb);
#pragma unroll
  for (int i = 0; i < NX17; ++i) { gx[i] += p[i]; a[i] = h3 * lam[i] + h2 * p[i]; p[i] = T(0); }
  f17_adj_lin<T, WP>(C + F17_LIN_N, u, M, P, a, p, gu, gtb);
#pragma unroll
  for (int i = 0; i < NX17; ++i) { gx[i] += p[i]; a[i] = h6 * lam[i] + h2 * p[i]; p[i] = T(0); }
  f17_adj_lin<T, WP>(C, u, M, P, a, p, gu, gtb);
#pragma unroll
  for (int i = 0; i < NX17; ++i) gx[i] += p[i];
}

// DPP row broadcast (v_mov_b32_dpp row_newbcast): lane L of every 16-lane row hands v to the row.
template <int L> __device__ __forceinline__ float rowbc(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x150 + L, 0xF, 0xF, true));
}
template <int L> __device__ __forceinline__ double rowbc(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_mov_dpp((int)b, 0x150 + L, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), 0x150 + L, 0xF, 0xF, true);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
// sin/cos of the five angles with 16 lanes per instance: lane t < 5 evaluates the pair of angle t
// and the row broadcast hands the ten values to the row
struct Trig17Row {
  int t;   // lane in the 16-lane row
  template <class T>
  __device__ __forceinline__ void operator()(const T* __restrict__ x, T (&sn)[5], T (&cs)[5]) const {
    const uint64_t m1 = lane_mask(t == 1), m2 = lane_mask(t == 2), m3 = lane_mask(t == 3), m4 = lane_mask(t == 4);
    T ang = csel(m1, x[4], x[3]);
    ang = csel(m2, x[5], ang);
    ang = csel(m3, x[12], ang);
    ang = csel(m4, x[13], ang);
    T s0, c0;
    sc(ang, &s0, &c0);
    sn[0] = rowbc<0>(s0); cs[0] = rowbc<0>(c0);
    sn[1] = rowbc<1>(s0); cs[1] = rowbc<1>(c0);
    sn[2] = rowbc<2>(s0); cs[2] = rowbc<2>(c0);
    sn[3] = rowbc<3>(s0); cs[3] = rowbc<3>(c0);
    sn[4] = rowbc<4>(s0); cs[4] = rowbc<4>(c0);
  }
};

// ---- the linearisation of one interval with 16 lanes per (instance, stage) --------------------
constexpr int LQ17 = 16, GQ17 = 64 / LQ17;

// One (instance, stage) of the packed linearisation, lane t < 16: column j of [A_k | B_k] into
// col(j, v[17]) and, on lane 0, the RK4 successor into succ(xn[17]).  Shared by the workspace
// kernel (lin17ws_kernel), the dense debug export (linearize17_kernel, mpcb_linearize) and the
// adjoint sweep of mpcb_eval (mpcb_eval.hip), so the parity test of mpcb_linearize covers the
// arithmetic the solver runs.
template <class T, class Col, class Succ>
__device__ __forceinline__ void lin17_packed(int t, const T* pb, T h, const Model<T>& M, const T* xk,
                                             const T* uk, Col&& colf, Succ&& succ) {
  if (t >= 14) {
    if (t == 14) {   // position and POC-state directions
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const int jj = q < 3 ? q : 11 + q;
        T v[NX17];
#pragma unroll
        for (int i = 0; i < NX17; ++i) v[i] = (i == jj) ? T(1) : T(0);
        colf(jj, v);
      }
    } else {         // velocity directions
      P17<T> P;
      unpack_p17(pb, P);
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) {
        const int jj = 6 + cc;
        T v[NX17];
#pragma unroll
        for (int i = 0; i < NX17; ++i) {
          v[i] = (i == jj) ? T(1) : T(0);
          if (i == cc) v[i] = h;
          if (i >= 14) v[i] = h * P.Jp[(i - 14) * 3 + cc];
        }
        colf(jj, v);
      }
    }
    return;
  }
  const int j = t < 3 ? 3 + t : (t < 8 ? 6 + t : 9 + t);   // 3..5, 9..13, 17..22
  P17<T> P;
  unpack_p17(pb, P);
  T x[NX17], u[NU17], dx[NX17], du[NU17], xn[NX17], col[NX17];
#pragma unroll
  for (int i = 0; i < NX17; ++i) {
    x[i] = xk[i];
    dx[i] = (j == i) ? T(1) : T(0);
  }
#pragma unroll
  for (int m = 0; m < NU17; ++m) {
    u[m] = uk[m];
    du[m] = (j == NX17 + m) ? T(1) : T(0);
  }
  // the five sin/cos of the nominal point: lane t < 5 of the row evaluates one (Trig17Row)
  rk4_17<T, true>(x, dx, u, du, h, M, P, xn, col, Trig17Row{t});
  colf(j, col);
  if (t == 0) succ(xn);
}

// Device-resident weights of the 17/6 OCP (row-major) and the default parameter vector.
template <class T>
struct Weights17 {
  T Q[NX17 * NX17];
  T R[NU17 * NU17];
  T QN[NX17 * NX17];
  T lbu[NU17], ubu[NU17];
  T lbx[NX17], ubx[NX17];   // state box on stages 1..N-1 (FullArgs::sbox)
  T p[NP17];
};

template <class T>
struct FullArgs {
  int64_t b0, nb;    // first global instance of the chunk, instances in the chunk
  int N, mode;
  T h, s;
  Model<T> M;
  const Weights17<T>* W;
  const T* p; int64_t p_sb, p_kb;   // parameters [B|1][N|1][25] (instance / stage strides, 0 =
                                   // broadcast); nullptr -> W->p
  const T* x0; int64_t x0_sb;
  const T* xref; int64_t xref_sb;
  const T* uref; int64_t uref_sb;
  const T* xbar; const T* ubar;
  T* u0; T* X; T* U; int32_t* status;
  T* ws;             // chunk workspace: per instance full17_elems(N) elements
  int box;           // input box lbu <= u <= ubu (interior-point iterations)
  int sbox;          // with box: state box lbx <= x_k <= ubx on stages 1..N-1
  int max_as_iter;   // iteration cap
  int32_t* qp_stats; // boxes: per instance [interior-point iterations, polish passes] (mpcb_qp_stats)
};

// Per-instance cost weights of the 17/6 calls (mpcb_solve_iterate_pw17, mpcb_solve_vjp_pw17): a
// second kernel argument of the PW kernels, so FullArgs / Vjp17Args and the shared-weight kernels
// stay as they are.  Row-major [17,17] / [6,6] / [17,17] at base + b * stride (elements; 0
// broadcasts).  Never null: the caller resolves a missing matrix to the handle's, stride 0.
template <class T>
struct Pw17 {
  const T* Q = nullptr;  int64_t Q_sb = 0;
  const T* R = nullptr;  int64_t R_sb = 0;
  const T* QN = nullptr; int64_t QN_sb = 0;
};

// The C API's weight arguments -> Pw17: NULL is the handle's matrix for every instance (stride 0,
// whatever stride came with the NULL).  False when all three are NULL: the shared-weight kernels.
template <class T>
inline bool resolve_pw17(const Weights17<T>* W, const void* Qw, int64_t Qw_sb, const void* Rw, int64_t Rw_sb,
                         const void* QNw, int64_t QNw_sb, Pw17<T>* out) {
  if (!Qw && !Rw && !QNw) return false;
  out->Q = Qw ? (const T*)Qw : W->Q;     out->Q_sb = Qw ? Qw_sb : 0;
  out->R = Rw ? (const T*)Rw : W->R;     out->R_sb = Rw ? Rw_sb : 0;
  out->QN = QNw ? (const T*)QNw : W->QN; out->QN_sb = QNw ? QNw_sb : 0;
  return true;
}

__host__ __device__ constexpr int64_t full17_elems(int N) {
  // XB (N+1)x17 | UB Nx6 | AB N x 23 columns x 17 | KR N x (6x17 + 6) | GP N x 17 |
  // boxes: DX, DDX (N+1)x17 | IP N x 18 | DDU N x 6 | IX (N+1) x 4 x 17 | LC N x 24 | DAX (N+1)x17 | DAU N x 6 | DC N x 48 | GV (N+1) x 24
  return (int64_t)(N + 1) * NX17 + (int64_t)N * (NU17 + NZ17 * NX17 + NU17 * NX17 + NU17 + NX17) +
         2 * (int64_t)(N + 1) * NX17 + (int64_t)N * (18 + NU17) + 4 * (int64_t)(N + 1) * NX17 +
         (int64_t)N * 24 + (int64_t)(N + 1) * NX17 + (int64_t)N * NU17 + (int64_t)N * 48 + (int64_t)(N + 1) * 24;
}

// n x n Cholesky (row-major H, lower L with 1/L_ii on the diagonal) and the solve L L^T x = b
template <class T, int n>
__device__ __forceinline__ void chol_n(const T* __restrict__ H, T* __restrict__ L) {
#pragma unroll
  for (int i = 0; i < n; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      T acc = H[i * n + j];
#pragma unroll
      for (int k = 0; k < j; ++k) acc -= L[i * n + k] * L[j * n + k];
      if (i == j) L[i * n + i] = inv_sqrt(acc);
      else L[i * n + j] = acc * L[j * n + j];
    }
  }
}
template <class T, int n>
__device__ __forceinline__ void chol_n_solve(const T* __restrict__ L, const T* __restrict__ b,
                                             T* __restrict__ x) {
  T y[n];
#pragma unroll
  for (int i = 0; i < n; ++i) {
    T acc = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) acc -= L[i * n + k] * y[k];
    y[i] = acc * L[i * n + i];
  }
#pragma unroll
  for (int i = n - 1; i >= 0; --i) {
    T acc = y[i];
#pragma unroll
    for (int k = i + 1; k < n; ++k) acc -= L[k * n + i] * x[k];
    x[i] = acc * L[i * n + i];
  }
}

// x[i] for a lane-dependent i < 17 without dynamic register indexing
template <class T> __device__ __forceinline__ T sel17(const T* x, int i) {
  const T lo = sel<16>(x, i & 15);
  return (i == 16) ? x[16] : lo;
}

// Per-instance workspace carve (FullArgs::ws, full17_elems(N) elements per instance).
template <class T>
struct Ws17 {
  T *XB, *UB, *AB, *KR, *GP;
  T *DX, *DDX, *IP, *DDU, *IX;
  static constexpr int KR_N = NU17 * NX17 + NU17;
  __device__ __forceinline__ Ws17(T* ws, int N) {
    XB = ws;                                     // [N+1][17] nominal states
    UB = XB + (int64_t)(N + 1) * NX17;           // [N][6]    nominal inputs
    AB = UB + (int64_t)N * NU17;                 // [N][23][17] column j of [A_k|B_k] at j*17
    KR = AB + (int64_t)N * NZ17 * NX17;          // [N][6*17 + 6]: K[m][i] at i*6 + m, then k
    GP = KR + (int64_t)N * KR_N;                 // [N][17] gaps
    // input box (interior point): iterate dx, step, (du, lambda_l, lambda_u), step du
    DX = GP + (int64_t)N * NX17;                 // [N+1][17]
    DDX = DX + (int64_t)(N + 1) * NX17;          // [N+1][17]
    IP = DDX + (int64_t)(N + 1) * NX17;          // [N][18]: du | lambda_l | lambda_u
    DDU = IP + (int64_t)N * 18;                  // [N][6]
    // state box: slacks and multipliers s_l | s_u | lambda_l | lambda_u of the rows of stage k
    IX = DDU + (int64_t)N * NU17;                // [N+1][4][17]
  }
};

// The Mehrotra arrays after IX (mpcb_r17.hip; a separate carve so the other 17/6 kernels keep
// their register footprint): the packed Cholesky factor of Huu per stage (21 of 24), the
// predictor's (affine) direction, and per row (z index: states, then 17 + m) w = 1/s_l - 1/s_u at
// [0, 24), c = Delta s_a Delta lambda_a / s_l - (upper) at [24, 48): the corrector's gradient
// change is c - sigma mu w.  GV: the predictor's stage gradients without the p terms (cost and
// barrier: states at [0, 17), inputs at [17, 23)), and p_N at stage N.
template <class T>
struct WsM17 {
  T *LC, *DAX, *DAU, *DC, *GV;
  static constexpr int LC_N = 24, DC_N = 48;
  __device__ __forceinline__ WsM17(const Ws17<T>& w, int N) {
    LC = w.IX + (int64_t)(N + 1) * 4 * NX17;     // [N][24]
    DAX = LC + (int64_t)N * LC_N;                // [N+1][17]
    DAU = DAX + (int64_t)(N + 1) * NX17;         // [N][6]
    DC = DAU + (int64_t)N * NU17;                // [N][48]
    GV = DC + (int64_t)N * DC_N;                 // [N+1][24]
  }
};

constexpr double IPM17_SIGMA_MIN = 0.05, IPM17_SIGMA_MAX = 0.9, IPM17_TAU = 0.995, IPM17_THETA = 0.1;
// (IPM17_BREAK: oracle.ocp.IPM_BREAK_TOL, where the choice of 1e-5 is explained: an fp64 exit
// there that the polish below does not certify ends MPCB_STATUS_MINSTEP, not OK)
constexpr double IPM17_TOL = 1e-12, IPM17_BREAK = 1e-5, IPM17_STALL = 1e-6, IPM17_RES = 1e-9;
// the fp64 state-box polish (oracle.ocp.al_polish): augmented-Lagrangian passes over the
// interior point's active set with one active-set change per pass
constexpr double POL17_RHO = 1e10, POL17_EQ = 1e-10, POL17_FEAS = 1e-10, POL17_ACT = 100.0;
constexpr int POL17_ITERS = 12;
// the state rows of the product (mpcb_solve_vjp17_sx): augmented-Lagrangian passes over the adjoint
// problem, the penalty SX17_RHO on the diagonal of every active state row.  1e8 and not the
// polish's 1e10: the product has no iterate to absorb the cancellation in P, and a weakly
// controllable row (a position row one stage ahead) still converges within SX17_ITERS passes
// (DESIGN.md has the measurement).  A pass ends an instance at eq <= SX17_EQ max(1, |dx|_inf).
#ifndef MPCB_SX17_RHO   // (-DMPCB_SX17_RHO=...: the variant builds of tools/sx_rho_sweep.py, nothing else)
#define MPCB_SX17_RHO 1e8
#endif
constexpr double SX17_RHO = MPCB_SX17_RHO, SX17_EQ = 1e-10;
constexpr int SX17_ITERS = 12;
constexpr double IPM17_SHORT = 1e-2;   // IPM17_SHORT_RUN steps in a row below it: a stalled QP
constexpr int IPM17_SHORT_RUN = 10;
// with the state box (the only QPs here that can be infeasible; oracle.ocp IPM_SBOX_SHORT): 7
// steps in a row below 0.05 away from the solution.  On the 4096 bench draws (N = 60) no
// LP-feasible instance takes more than 3 such steps in a row, the 68 LP-infeasible ones stop
// after at most 69 iterations instead of 115 (the launch's tail: feasible ones need <= 62)
constexpr double IPM17_SBOX_SHORT = 5e-2;
constexpr int IPM17_SBOX_SHORT_RUN = 7;
// fp32: the duality measure stops near 1e-6 (lambda / s reaches the fp32 conditioning limit
// long before 1e-12), so the tolerances scale with the precision; the result is checked
// against the fp64 oracle in tests/test_gpu_full17.py
constexpr double IPM17_TOL_F32 = 1e-6, IPM17_BREAK_F32 = 1e-3, IPM17_RES_F32 = 1e-5;

// ---- mpcb_solve_vjp17 (mpcb_r17.hip): the vector-Jacobian product of the 17/6 RTI step ---------
template <class T>
struct Vjp17Args {
  int64_t b0, nb;    // first global instance of the chunk, instances in the chunk
  int N;
  T h, s;
  Model<T> M;
  const Weights17<T>* W;
  const T* p; int64_t p_sb, p_kb;   // parameters as FullArgs; nullptr -> W->p
  const T* xbar; const T* ubar;     // the linearisation point
  const uint8_t* fixed;             // [B][N][6] nonzero = clamped (nullable: nothing clamped)
  const T* X; const T* U;           // weight gradients only: the solve's output ...
  const T* xref; int64_t xref_sb;   // ... and its references
  const T* uref; int64_t uref_sb;
  const T* gX; const T* gU;         // cotangents (one may be null)
  T* gx0; T* gxref; T* guref;
  T* gQ; T* gR; T* gQN;
  int32_t* status;
  T* ws;             // the call's own chunk workspace: per instance vjp17_elems(N) elements
};

// Per-instance workspace carve of the product (Vjp17Args::ws): the linearisation in Ws17::AB's
// column layout, the gains in Ws17::KR's, the adjoint trajectory (dx, du) for the weight sums, a
// sink of the same shape as (gxref, guref) for the stores of outputs nobody asked for, and one
// check value per stage from the linearisation kernel (0, or NaN for a non-finite input), and the
// multiplier estimates of the state rows (vjp17_sx kernels only).
__host__ __device__ constexpr int64_t vjp17_elems(int N) {
  return (int64_t)N * (NZ17 * NX17 + NU17 * NX17 + NU17) + 2 * ((int64_t)(N + 1) * NX17 + (int64_t)N * NU17) + N +
         (int64_t)(N + 1) * NX17;
}
template <class T>
struct WsV17 {
  T *AB, *KR, *DX, *DU, *SK, *CK, *NU;
  __device__ __forceinline__ WsV17(T* ws, int N) {
    AB = ws;                                     // [N][23][17]
    KR = AB + (int64_t)N * NZ17 * NX17;          // [N][6*17 + 6]
    DX = KR + (int64_t)N * Ws17<T>::KR_N;        // [N+1][17]
    DU = DX + (int64_t)(N + 1) * NX17;           // [N][6]
    SK = DU + (int64_t)N * NU17;                 // [N+1][17] | [N][6]
    CK = SK + (int64_t)(N + 1) * NX17 + (int64_t)N * NU17;   // [N]
    NU = CK + N;                                 // [N+1][17]
  }
};
template <class T> hipError_t launch_vjp17(const Vjp17Args<T>& a, hipStream_t st);

// ---- mpcb_solve_gains on the 17/6 model (mpcb_r17.hip): the linearisation kernel of the product
// above, on its workspace, then the backward pass that stores K_k and P_0.  Of `v` the chunk, the
// model, the weights, the parameters, (xbar, ubar), fixed, status and ws are read.
template <class T>
struct Gains17Args {
  Vjp17Args<T> v;
  T* K; T* P0;       // [B][N][6][17], [B][17][17], either nullable
};
template <class T> hipError_t launch_gains17(const Gains17Args<T>& a, hipStream_t st);

// ev (nullable): 4 events recorded before nominal17, after it, after lin17ws and after riccati17.
template <class T> hipError_t launch_full17(const FullArgs<T>& a, hipStream_t st, hipEvent_t* ev = nullptr);
template <class T> hipError_t launch_riccati17q(const FullArgs<T>& a, hipStream_t st);
// The per-instance-weight pipeline: the same three kernels by plain launches (no launch log, no
// events), the Riccati kernel's PW variant when pw is given; pw == nullptr: the shared-weight one.
template <class T> hipError_t launch_full17_pw(const FullArgs<T>& a, const Pw17<T>* pw, hipStream_t st);
template <class T> hipError_t launch_riccati17q_pw(const FullArgs<T>& a, const Pw17<T>* pw, hipStream_t st);
template <class T> hipError_t launch_vjp17_pw(const Vjp17Args<T>& a, const Pw17<T>& pw, hipStream_t st);
// mpcb_solve_vjp17_sx: the product with active state rows (fixed_x [B][N+1][17], nonzero = active,
// never null; a kernel argument of its own, so Vjp17Args and the kernels above stay as they are),
// fp64 only; pw == nullptr: the handle's weights.
hipError_t launch_vjp17_sx(const Vjp17Args<double>& a, const Pw17<double>* pw, const uint8_t* fixed_x,
                           hipStream_t st);
template <class T>
hipError_t launch_linearize17(int64_t B, int N, T h, const Model<T>& M, const T* p, int64_t p_sb,
                              int64_t p_kb, const T* xbar, const T* ubar, T* A, T* Bm, T* xnext, hipStream_t st);
template <class T>
hipError_t launch_sim_step17(int64_t B, T h, const Model<T>& M, const T* p, int64_t p_sb,
                             const T* x, const T* u, T* xo, hipStream_t st);
// mpcb_sim_step_vjp17 (mpcb_simvjp17.hip): the reverse sweep of that step.  p is never null (the
// caller resolves the handle's array or the defaults); any output may be null.
template <class T>
hipError_t launch_sim_step_vjp17(int64_t B, T h, const Model<T>& M, const T* p, int64_t p_sb, const T* x,
                                 const T* u, const T* gxn, T* gx, T* gu, T* gparams, hipStream_t st);
template <class T> hipError_t launch_eval17(const EvalArgs<T>& a, hipStream_t st);   // mpcb_eval.hip

}  // namespace mpcb
