// Per-env quadrotor math for the fused step kernel (gfx950, one env per lane).
//
// Everything here is register-resident f32 scalar code: 3x3 / 4x4 / 9x9 work is
// far too small for MFMA (no dense contraction on this path), so it
// is written as straight-line VALU math that the compiler keeps in VGPRs.
//
// Each function names the reference routine it restates.  Where the reference
// evaluates an ill-conditioned Kalman update literally — (I - K H) P with
// R = 1e-7 against P = O(1..1000) — the algebraically identical, f32-stable
// form is used instead (derivations in DESIGN.md §4); the literal float64 form
// lives in the CPU oracle, pinned against the reference's own modules.
#pragma once
#ifdef OUZ_HOST
#include "host_compat.h"   // the host build of the step (quad_host.cpp)
#else
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include <type_traits>

#include "philox.h"

// The probe build of the kernels (-DOUZ_STAMPS) defines OUZ_STAMP before this file; every other build stamps nothing.
#ifdef OUZ_STAMP
#define OUZ_SUBSTEP_STAMP(k) OUZ_STAMP(k, false)
#else
#define OUZ_SUBSTEP_STAMP(k) do {} while (0)
#endif

namespace ouz {

// ---------------------------------------------------------------------------
// small vector / matrix types
// ---------------------------------------------------------------------------
struct V3 { float x, y, z; };
struct Q4 { float x, y, z, w; };          // xyzw (Isaac root-state order)
template <typename T>
struct M3T { T m[9]; };                    // row-major
using M3 = M3T<float>;

OUZ_HD V3 v3(float x, float y, float z) { return V3{x, y, z}; }
OUZ_HD V3 operator+(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
OUZ_HD V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
OUZ_HD V3 operator*(float s, V3 a) { return V3{s * a.x, s * a.y, s * a.z}; }
OUZ_HD V3 mul(V3 a, V3 b) { return V3{a.x * b.x, a.y * b.y, a.z * b.z}; }
OUZ_HD float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
OUZ_HD V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
OUZ_HD float norm(V3 a) { return sqrtf(dot(a, a)); }

OUZ_HD V3 mv(const M3& A, V3 v) {
  return V3{A.m[0] * v.x + A.m[1] * v.y + A.m[2] * v.z, A.m[3] * v.x + A.m[4] * v.y + A.m[5] * v.z,
            A.m[6] * v.x + A.m[7] * v.y + A.m[8] * v.z};
}
OUZ_HD V3 mtv(const M3& A, V3 v) {  // A^T v
  return V3{A.m[0] * v.x + A.m[3] * v.y + A.m[6] * v.z, A.m[1] * v.x + A.m[4] * v.y + A.m[7] * v.z,
            A.m[2] * v.x + A.m[5] * v.y + A.m[8] * v.z};
}
// A (3x3) times the 3-vector a[0..2], into out[0..2]
template <typename T>
OUZ_HD void mva(const M3T<T>& A, const T* a, T* out) {
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = A.m[i * 3 + 0] * a[0] + A.m[i * 3 + 1] * a[1] + A.m[i * 3 + 2] * a[2];
}
template <typename T>
OUZ_HD M3T<T> mm(const M3T<T>& A, const M3T<T>& B) {
  M3T<T> C;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      C.m[i * 3 + j] = A.m[i * 3 + 0] * B.m[0 * 3 + j] + A.m[i * 3 + 1] * B.m[1 * 3 + j] + A.m[i * 3 + 2] * B.m[2 * 3 + j];
  return C;
}
template <typename T>
OUZ_HD M3T<T> mmt(const M3T<T>& A, const M3T<T>& B) {  // A B^T
  M3T<T> C;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      C.m[i * 3 + j] = A.m[i * 3 + 0] * B.m[j * 3 + 0] + A.m[i * 3 + 1] * B.m[j * 3 + 1] + A.m[i * 3 + 2] * B.m[j * 3 + 2];
  return C;
}
template <typename T>
OUZ_HD M3T<T> tr(const M3T<T>& A) {
  M3T<T> C;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C.m[i * 3 + j] = A.m[j * 3 + i];
  return C;
}
// 1 / x.  On the device, f64: the hardware reciprocal estimate refined by two Newton steps (full
// double precision for the normal, positive determinants of SPD 3x3 blocks) instead of the
// correctly rounded division sequence (div_scale / div_fmas / div_fixup), ~2x fewer f64 issues.
template <typename T>
OUZ_HD T recip(T x) {
#ifdef __HIP_DEVICE_COMPILE__
  if constexpr (std::is_same_v<T, double>) {
    double y = __builtin_amdgcn_rcp(x);
    y = y * (2.0 - x * y);
    return y * (2.0 - x * y);
  }
#endif
  return T(1) / x;
}

// 1 / sqrt(x) for x > 0.  On the device, f64: the hardware estimate refined by two Newton steps (full double
// precision) instead of the correctly rounded sqrt sequence followed by a division.
template <typename T>
OUZ_HD T rsqrt_r(T x) {
#ifdef __HIP_DEVICE_COMPILE__
  if constexpr (std::is_same_v<T, double>) {
    double y = __builtin_amdgcn_rsq(x);
    double h = 0.5 * x;
    y = y * (1.5 - h * y * y);
    return y * (1.5 - h * y * y);
  }
#endif
  return T(1) / sqrt(x);
}

// ---------------------------------------------------------------------------
// rotations
// ---------------------------------------------------------------------------
// quaternion_to_matrix on the wxyz reorder of an xyzw quaternion
// (controllers/rotation_conversions.py:36-64; position_control.py:28-29).
OUZ_HD M3 quat_to_mat(Q4 q) {
  float r = q.w, i = q.x, j = q.y, k = q.z;
  float two_s = 2.0f / (r * r + i * i + j * j + k * k);
  return M3{{1.0f - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
             two_s * (i * j + k * r), 1.0f - two_s * (i * i + k * k), two_s * (j * k - i * r),
             two_s * (i * k - j * r), two_s * (j * k + i * r), 1.0f - two_s * (i * i + j * j)}};
}

// matrix_to_euler_angles(R, "ZYX")[:, [2,1,0]] (rotation_conversions.py:216-255):
// roll = atan2(R21, R22), pitch = asin(-R20), yaw = atan2(R10, R00).
// The controllers only consume sin/cos of these angles (position_control.py:51-52,75-79),
// so they are formed directly from R: cos(atan2(y, x)) = x / hypot(x, y), etc. — the
// same numbers without 2 atan2 + 1 asin + 6 sin/cos per env.  Only the position
// controller needs the yaw angle itself (its yaw-rate error, :89-92).
struct EulerSC { float sr, cr, sp, cp, sy, cy; };

// Selects, not a branch: the quotient is formed for every lane and 0 * inf is discarded where h2 == 0, so the
// values are the branch form's and the controller around the two calls stays one basic block.
OUZ_HD void unit2(float y, float x, float& s, float& c) {
  const float h2 = x * x + y * y;
  const bool ok = h2 > 0.0f;
  const float ih = 1.0f / sqrtf(h2);
  s = ok ? y * ih : 0.0f;     // atan2(0, 0) = 0
  c = ok ? x * ih : 1.0f;
}

OUZ_HD EulerSC euler_sc(const M3& R) {
  EulerSC e;
  unit2(R.m[7], R.m[8], e.sr, e.cr);
  e.sp = -R.m[6];
  e.cp = sqrtf(fmaxf(0.0f, 1.0f - R.m[6] * R.m[6]));   // cos(asin(x)) >= 0
  unit2(R.m[3], R.m[0], e.sy, e.cy);
  return e;
}

OUZ_HD void mat_to_rpy(const M3& R, float& roll, float& pitch, float& yaw) {
  roll = atan2f(R.m[7], R.m[8]);
  pitch = asinf(-R.m[6]);
  yaw = atan2f(R.m[3], R.m[0]);
}

// euler_angles_to_matrix((yaw, pitch, roll), "ZYX") = Rz Ry Rx from sines/cosines.
OUZ_HD M3 rpy_to_mat_sc(float cz, float sz, float cy, float sy, float cx, float sx) {
  return M3{{cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx, sz * cy, sz * sy * sx + cz * cx,
             sz * sy * cx - cz * sx, -sy, cy * sx, cy * cx}};
}

// euler_angles_to_matrix((yaw, pitch, roll), "ZYX") = Rz Ry Rx (rotation_conversions.py:149-171).
OUZ_HD M3 rpy_to_mat(float yaw, float pitch, float roll) {
  return rpy_to_mat_sc(cosf(yaw), sinf(yaw), cosf(pitch), sinf(pitch), cosf(roll), sinf(roll));
}

// my_quat_rotate / quat_rotate, xyzw (utils/torch_jit_utils.py:198-208).
OUZ_HD V3 quat_rotate(Q4 q, V3 v) {
  V3 qv = v3(q.x, q.y, q.z);
  V3 a = (2.0f * q.w * q.w - 1.0f) * v;
  V3 b = (q.w * 2.0f) * cross(qv, v);
  V3 c = (dot(qv, v) * 2.0f) * qv;
  return a + b + c;
}

OUZ_HD Q4 quat_mul(Q4 a, Q4 b) {  // xyzw Hamilton product a (x) b
  return Q4{a.w * b.x + b.w * a.x + (a.y * b.z - a.z * b.y), a.w * b.y + b.w * a.y + (a.z * b.x - a.x * b.z),
            a.w * b.z + b.w * a.z + (a.x * b.y - a.y * b.x), a.w * b.w - (a.x * b.x + a.y * b.y + a.z * b.z)};
}

// ---------------------------------------------------------------------------
// Lee geometric controllers
// ---------------------------------------------------------------------------
struct LeeGains { V3 kP, kV, kR, kW; };

OUZ_HD LeeGains default_gains() {  // controllers/control_config.py:14-17
  return LeeGains{v3(0.8f, 0.8f, 1.0f), v3(0.5f, 0.5f, 0.4f), v3(3.0f, 3.0f, 1.0f), v3(0.5f, 0.5f, 1.2f)};
}

constexpr float kTwoPiF = 6.28318530717958647692f;
constexpr float kPiF = 3.14159265358979323846f;

// torch.remainder for floats: fmod, then shift into the divisor's sign.  fmod(a, b) == a
// exactly when |a| < b, which is the common case here (a = yaw command - yaw); only larger
// arguments pay for the libm fmodf.
OUZ_HD float remainder_f(float a, float b) {
  float m = (fabsf(a) < b) ? a : fmodf(a, b);
  if (m != 0.0f && ((b < 0.0f) != (m < 0.0f))) m += b;
  return m;
}
// remainder_f under the precondition |a| < b (or a NaN): fmod(a, b) is a itself, so only the sign shift is left.
OUZ_HD float remainder_small_f(float a, float b) {
  float m = a;
  if (m != 0.0f && ((b < 0.0f) != (m < 0.0f))) m += b;
  return m;
}

// atan2f under the precondition that x and y are finite with |x|, |y| <= 2^96 (the zero-yaw controller's arguments
// are R10 and R00 of a normalised quaternion: magnitude at most 1 plus rounding).  On the device: the library
// routine's own operations in its order (the quotient min * rcp(max), its eight-coefficient series in the squared
// quotient, the octant folds, the y == 0 case, the sign of y) without its 2^96 range scaling, its both-infinite
// case and its unordered case, which the precondition rules out: bit for bit atan2f there, one basic block.
// Outside the precondition (infinities, NaN, larger magnitudes) the value is unspecified.  The host keeps atan2f.
OUZ_HD float atan2_bounded_f(float y, float x) {
#if defined(OUZ_HOST) || !defined(__HIP_DEVICE_COMPILE__)
  return atan2f(y, x);
#else
  const float ax = fabsf(x), ay = fabsf(y);
  const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
  const float v = mn * __builtin_amdgcn_rcpf(mx);
  const float t = v * v;
  float s = fmaf(t, __uint_as_float(0x3b2d2a58u), __uint_as_float(0xbc7a590cu));
  s = fmaf(t, s, __uint_as_float(0x3d29fb3fu));
  s = fmaf(t, s, __uint_as_float(0xbd97d4d7u));
  s = fmaf(t, s, __uint_as_float(0x3dd931b2u));
  s = fmaf(t, s, __uint_as_float(0xbe1160e6u));
  s = fmaf(t, s, __uint_as_float(0x3e4cb8bfu));
  s = fmaf(t, s, __uint_as_float(0xbeaaaa62u));
  const float ts = t * s;
  float a = fmaf(v, ts, v);
  a = ay > ax ? __uint_as_float(0x3fc90fdbu) - a : a;                                    // pi/2 - a
  a = x < 0.0f ? __uint_as_float(0x40490fdbu) - a : a;                                   // pi - a
  const float a0 = (int)__float_as_uint(x) < 0 ? __uint_as_float(0x40490fdbu) : 0.0f;    // y == 0: pi or 0 by x's sign bit
  a = y == 0.0f ? a0 : a;
  return __builtin_copysignf(a, y);
#endif
}

// Shared attitude loop (position_control.py:66-108): returns torque.
OUZ_HD V3 lee_attitude_loop(const M3& R, const M3& Rd, V3 omega, const EulerSC& e, float yaw_rate,
                            const LeeGains& g) {
  // A = Rd^T R ; vee(A - A^T) = (A21 - A12, A02 - A20, A10 - A01)
  M3 A;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      A.m[i * 3 + j] = Rd.m[0 * 3 + i] * R.m[0 * 3 + j] + Rd.m[1 * 3 + i] * R.m[1 * 3 + j] + Rd.m[2 * 3 + i] * R.m[2 * 3 + j];
  V3 e_R = v3(0.5f * (A.m[7] - A.m[5]), 0.5f * (A.m[2] - A.m[6]), 0.5f * (A.m[3] - A.m[1]));
  // omega_d = E (0, 0, yaw_rate), E = rotmat_euler_to_body_rates (:73-86)
  V3 wd = v3(-e.sp * yaw_rate, e.sr * e.cp * yaw_rate, e.cr * e.cp * yaw_rate);
  V3 des = mtv(A, wd);   // R^T Rd wd = (Rd^T R)^T wd
  V3 act = mtv(R, omega);
  V3 e_w = act - des;
  // + cross(w, w) == 0 (position_control.py:108)
  return v3(-g.kR.x * e_R.x - g.kW.x * e_w.x, -g.kR.y * e_R.y - g.kW.y * e_w.y, -g.kR.z * e_R.z - g.kW.z * e_w.z);
}

// LeePositionController.__call__ (controllers/position_control.py:19-109).
// cmd = (x, y, z, yaw); thrust in units of m*g, torque "inertia normalised".
// R = quat_to_mat(q) of the state quaternion (the step kernel shares it with the integrator).
// kZeroYaw: the caller passes cmd_yaw == 0 (every step path).  Then the yaw error is -atan2f(..), |atan2f| <= pi_f32 <
// 2 pi_f32, and the remainder needs no fmodf: the same value without the libm expansion (two loops, an f64 convert)
// sitting between the yaw and the controller body.  The C-ABI controller entry takes any yaw command: false.
template <bool kZeroYaw = false>
OUZ_HD void lee_position_R(const M3& R, V3 p, V3 v, V3 w, V3 cmd_p, float cmd_yaw, const LeeGains& g,
                           float& thrust, V3& torque) {
  EulerSC e = euler_sc(R);
  V3 a = mul(g.kP, cmd_p - p) - mul(g.kV, v);
  a.z += 1.0f;
  thrust = a.x * R.m[2] + a.y * R.m[5] + a.z * R.m[8];
  V3 b3 = (1.0f / norm(a)) * a;
  V3 b2 = cross(b3, v3(e.cy, e.sy, 0.0f));
  b2 = (1.0f / norm(b2)) * b2;
  V3 b1 = cross(b2, b3);
  M3 Rd{{b1.x, b2.x, b3.x, b1.y, b2.y, b3.y, b1.z, b2.z, b3.z}};
  const float ya = cmd_yaw - (kZeroYaw ? atan2_bounded_f(R.m[3], R.m[0]) : atan2f(R.m[3], R.m[0]));
  float yr = kZeroYaw ? remainder_small_f(ya, kTwoPiF) : remainder_f(ya, kTwoPiF);
  if (yr > kPiF) yr -= kTwoPiF;
  torque = lee_attitude_loop(R, Rd, w, e, yr, g);
}

OUZ_HD void lee_position(V3 p, Q4 q, V3 v, V3 w, V3 cmd_p, float cmd_yaw, const LeeGains& g, float& thrust,
                         V3& torque) {
  lee_position_R(quat_to_mat(q), p, v, w, cmd_p, cmd_yaw, g, thrust, torque);
}

// LeeVelocityController.__call__ (controllers/velocity_control.py:17-112).
OUZ_HD void lee_velocity(Q4 q, V3 v, V3 w, V3 cmd_v, float yaw_rate, const LeeGains& g, float& thrust,
                         V3& torque) {
  M3 R = quat_to_mat(q);
  EulerSC e = euler_sc(R);
  // vehicle frame Rz(yaw): v_vehicle = Rz^T v
  V3 vv = v3(e.cy * v.x + e.sy * v.y, -e.sy * v.x + e.cy * v.y, v.z);
  V3 a = mul(g.kV, cmd_v - vv);
  a.z += 1.0f;
  thrust = a.x * R.m[2] + a.y * R.m[5] + a.z * R.m[8];
  // pitch_sp = atan2(a0, a2), roll_sp = atan2(-a1, hypot(a0, a2)) (:58-60) as sin/cos
  float spt, cpt, srl, crl;
  unit2(a.x, a.z, spt, cpt);
  unit2(-a.y, sqrtf(a.z * a.z + a.x * a.x), srl, crl);
  M3 Rd = rpy_to_mat_sc(e.cy, e.sy, cpt, spt, crl, srl);
  torque = lee_attitude_loop(R, Rd, w, e, yaw_rate, g);
}

// LeeAttitudeContoller.__call__ (controllers/attitude_control.py:17-78): cmd = (T, roll, pitch, yaw_rate).
OUZ_HD void lee_attitude(Q4 q, V3 w, float cmd_t, float cmd_roll, float cmd_pitch, float yaw_rate,
                         const LeeGains& g, float& thrust, V3& torque) {
  M3 R = quat_to_mat(q);
  EulerSC e = euler_sc(R);
  M3 Rd = rpy_to_mat_sc(e.cy, e.sy, cosf(cmd_pitch), sinf(cmd_pitch), cosf(cmd_roll), sinf(cmd_roll));
  torque = lee_attitude_loop(R, Rd, w, e, yaw_rate, g);
  thrust = cmd_t + 1.0f;
}

// ---------------------------------------------------------------------------
// AHRS-EKF, executed "ang" branch (ahrs_ekf.py:1301-1337), SURVEY a12.
// q = (w, x, y, z) scalar-first; P symmetric 4x4 packed (00,01,02,03,11,12,13,22,23,33).
// ---------------------------------------------------------------------------
struct EkfQ { float w, x, y, z; };

OUZ_HD int s4(int i, int j) {  // packed index, any order
  int a = i < j ? i : j, b = i < j ? j : i;
  return a * 4 - (a * (a - 1)) / 2 + (b - a);
}

// Full symmetric 4x4 inverse via Cholesky (S is SPD: P_t + 1e-7 I), in R.  The pivots L[j][j] are only ever used
// through their inverses (the off-diagonal sums and Linv run over k < j), so each is one reciprocal square root.
template <typename R>
OUZ_HD void inv_spd4(const R S[10], R Si[10]) {
  R L[4][4] = {};
  R Ld[4];   // 1 / L[j][j]
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    R d = S[s4(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    const R inv = rsqrt_r(d);
    Ld[j] = inv;
#pragma unroll
    for (int i = j + 1; i < 4; ++i) {
      R s = S[s4(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s * inv;
    }
  }
  // Linv (lower)
  R Li[4][4] = {};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    Li[i][i] = Ld[i];
#pragma unroll
    for (int j = 0; j < i; ++j) {
      R s = R(0);
#pragma unroll
      for (int k = j; k < i; ++k) s += L[i][k] * Li[k][j];
      Li[i][j] = -s * Li[i][i];
    }
  }
  // S^-1 = Linv^T Linv
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j) {
      R s = R(0);
#pragma unroll
      for (int k = j; k < 4; ++k) s += Li[k][i] * Li[k][j];
      Si[s4(i, j)] = s;
    }
}

constexpr float kEkfGNoise = 0.09f;   // 0.3**2, ahrs_ekf.py:1004
constexpr float kEkfAngR = 1e-7f;      // ahrs_ekf.py:1332

// The EKF update is evaluated in EkfReal and stored in f32 (q, P), like the PV step: the reference's EKF is
// numpy float64 (ahrs_ekf.py:1280-1337).  float restores the round-4 f32 evaluation (an A/B build: -DOUZ_EKF_F32).
#ifdef OUZ_EKF_F32
typedef float EkfReal;
#else
typedef double EkfReal;
#endif

// In: q (normalised prior), P. Out: q, P updated in place.  Constants are the reference's Python floats (f64):
// 0.5 * Dt with Dt = 1 / frequency, g_noise = 0.3 ** 2, the 1e-7 measurement noise.
template <typename R>
OUZ_HD void ekf_update_t(EkfQ& q, float Pf[10], V3 gf, EkfQ ang, float Dt) {
  const R h = R(0.5) * R(Dt);
  const R gx = gf.x, gy = gf.y, gz = gf.z;
  const R r = sizeof(R) == 8 ? R(1e-7) : R(kEkfAngR);
  const R gnoise = sizeof(R) == 8 ? R(0.09) : R(kEkfGNoise);
  R P[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) P[k] = (R)Pf[k];
  // Omega(x) rows (ahrs_ekf.py:1072-1106)
  const R O[4][4] = {{R(0), -gx, -gy, -gz}, {gx, R(0), gz, -gy}, {gy, -gz, R(0), gx}, {gz, gy, -gx, R(0)}};
  const R qv[4] = {(R)q.w, (R)q.x, (R)q.y, (R)q.z};
  R qt[4];
  R F[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    R s = R(0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      R fij = (i == j ? R(1) : R(0)) + h * O[i][j];   // f(): (I + 0.5 Dt Omega(g)) q
      s += fij * qv[j];
      F[i][j] = (i == j ? R(1) : R(0)) + O[i][j] * h;  // dfdq: I + Omega(0.5 Dt g)
    }
    qt[i] = s;
  }
  // W = 0.5 Dt [ -q_v^T ; q_w I + skew(q_v) ]   (4x3), Q_t = 0.5 Dt g_noise W W^T
  R W[4][3] = {{-qv[1], -qv[2], -qv[3]}, {qv[0], -qv[3], qv[2]}, {qv[3], qv[0], -qv[1]}, {-qv[2], qv[1], qv[0]}};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) W[i][j] *= h;
  // FP (4x4 full)
  R FP[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      R s = R(0);
#pragma unroll
      for (int k = 0; k < 4; ++k) s += F[i][k] * P[s4(k, j)];
      FP[i][j] = s;
    }
  R Pt[10];
  const R qs = h * gnoise;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j) {
      R s = R(0);
#pragma unroll
      for (int k = 0; k < 4; ++k) s += FP[i][k] * F[j][k];
      R ww = W[i][0] * W[j][0] + W[i][1] * W[j][1] + W[i][2] * W[j][2];
      Pt[s4(i, j)] = s + qs * ww;
    }
  // S = P_t + r I ; stable identities:
  //   (I - K) P_t = r I - r^2 S^-1 ,  q_t + K v = ang - r S^-1 v
  R S[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) S[k] = Pt[k];
  S[s4(0, 0)] += r; S[s4(1, 1)] += r; S[s4(2, 2)] += r; S[s4(3, 3)] += r;
  R Si[10];
  inv_spd4<R>(S, Si);
  const R av[4] = {(R)ang.w, (R)ang.x, (R)ang.y, (R)ang.z};
  const R vv[4] = {av[0] - qt[0], av[1] - qt[1], av[2] - qt[2], av[3] - qt[3]};
  R qn[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    R s = R(0);
#pragma unroll
    for (int j = 0; j < 4; ++j) s += Si[s4(i, j)] * vv[j];
    qn[i] = av[i] - r * s;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j) Pf[s4(i, j)] = (float)((i == j ? r : R(0)) - (r * r) * Si[s4(i, j)]);
  const R inv = rsqrt_r(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3]);
  q = EkfQ{(float)(qn[0] * inv), (float)(qn[1] * inv), (float)(qn[2] * inv), (float)(qn[3] * inv)};
}

OUZ_HD void ekf_update(EkfQ& q, float P[10], V3 g, EkfQ ang, float Dt) { ekf_update_t<EkfReal>(q, P, g, ang, Dt); }

// ---------------------------------------------------------------------------
// Position/velocity KF (PVFilter.py:25-110), SURVEY a13.
// x = [p, v, b_a]; P symmetric 9x9 packed upper triangle (45 floats).
// ---------------------------------------------------------------------------
OUZ_HD constexpr int s9(int i, int j) {
  return (i <= j) ? (i * 9 - (i * (i - 1)) / 2 + (j - i)) : (j * 9 - (j * (j - 1)) / 2 + (i - j));
}

constexpr float kPvAccVar = 1.0f;     // [0.01]*3 * 100 (ekf_lee_landed.py:137)
constexpr float kPvPosVar = 1e-7f;    // ekf_lee_landed.py:408
constexpr float kPvP0 = 1000.0f;      // PVFilter.py:12

// The PV step's element formulas.  Every entry the step computes is ONE chain of explicit
// fmas in a fixed order, written once below and evaluated by two data layouts:
//  * the one-lane form (pv_predict_t / pv_correct_t): the packed covariance in one lane's registers -- the
//    large-N step kernels and the component entries;
//  * the quad-lane form (quad_pv_ql.h): the four lanes of an env split every 3x3 block by column, the full
//    symmetric covariance in LDS -- the latency-regime estimator kernels.
// Both take the same operations on the same operands for every stored element, so they agree bit for bit
// (contraction is off here: a * b + c is never fused behind the formulas' back).
template <typename T>
OUZ_HD T dot3(T a0, T a1, T a2, T b0, T b1, T b2) {   // a . b, the a0 * b0 product seeding the chain
#pragma clang fp contract(off)
  return fma(a2, b2, fma(a1, b1, a0 * b0));
}
template <typename T>
OUZ_HD T dot3s(T a0, T a1, T a2, T b0, T b1, T b2, T seed) {   // seed + a . b
#pragma clang fp contract(off)
  return fma(a2, b2, fma(a1, b1, fma(a0, b0, seed)));
}

// Inverse of a symmetric 3x3 via the adjugate (SPD inputs only).  Reads only the upper triangle.
template <typename T>
OUZ_HD M3T<T> inv_sym3(const M3T<T>& S) {
#pragma clang fp contract(off)
  const T a = S.m[0], b = S.m[1], c = S.m[2], d = S.m[4], e = S.m[5], f = S.m[8];
  const T A = fma(d, f, -(e * e)), B = fma(c, e, -(b * f)), C = fma(b, e, -(c * d));
  const T D = fma(a, f, -(c * c)), E = fma(b, c, -(a * e)), F = fma(a, d, -(b * b));
  const T inv_det = recip<T>(fma(c, C, fma(b, B, a * A)));
  return M3T<T>{{A * inv_det, B * inv_det, C * inv_det, B * inv_det, D * inv_det, E * inv_det,
                 C * inv_det, E * inv_det, F * inv_det}};
}

// M = R(q/|q|)^T, formed in f32 from the f32 quaternion as the reference's torch f32 does (PVFilter.py:31-35)
template <typename T>
OUZ_HD M3T<T> pv_rot(EkfQ q) {
  const float inv = 1.0f / sqrtf(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  const M3 Mf = tr(quat_to_mat(Q4{q.x * inv, q.y * inv, q.z * inv, q.w * inv}));
  M3T<T> M;
#pragma unroll
  for (int k = 0; k < 9; ++k) M.m[k] = (T)Mf.m[k];
  return M;
}

// prediction_step, state part: x = F x + G (a - b), F = [[I, M dt, M h],[0, M, M dt],[0, 0, I]], h = dt^2 / 2
template <typename T>
OUZ_HD void pv_state_predict(T x[9], const T acc[3], const M3T<T>& M, T dt, T h) {
#pragma clang fp contract(off)
  T a1[3], a2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const T u = acc[k] - x[6 + k];
    a1[k] = fma(h, u, fma(dt, x[3 + k], h * x[6 + k]));   // -> position
    a2[k] = fma(dt, u, fma(dt, x[6 + k], x[3 + k]));      // -> velocity
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) x[i] += dot3(M.m[i * 3], M.m[i * 3 + 1], M.m[i * 3 + 2], a1[0], a1[1], a1[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) x[3 + i] = dot3(M.m[i * 3], M.m[i * 3 + 1], M.m[i * 3 + 2], a2[0], a2[1], a2[2]);
}

// prediction_step, covariance part, P' = F P F^T + q_a G G^T, by columns.  With X_{r,b} the 3x3 blocks of P and
// G_{r,b} = (F P)_{r,b}:  G_{0,b} = X_{0,b} + M (dt X_{1,b} + h X_{2,b}),  G_{1,b} = M (X_{1,b} + dt X_{2,b}),
// G_{2,b} = X_{2,b};  then with Z00 = dt G_{0,1} + h G_{0,2}, Z01 = G_{0,1} + dt G_{0,2}, Z11 = G_{1,1} + dt G_{1,2}:
//   P'_00 = G_{0,0} + Z00 M^T + q h^2 I,   P'_01 = Z01 M^T + q h dt I,   P'_11 = Z11 M^T + q dt^2 I,
//   P'_02 = G_{0,2},   P'_12 = G_{1,2},   P'_22 = X_{2,2}
// (G Q G^T = q_a [[h^2 M M^T, h dt M M^T], [dt h M M^T, dt^2 M M^T]] with M M^T = I up to M's f32 rounding,
// the same as in the reference's own f32 product: the noise is diagonal).  Column c of G_{r,b} needs only
// column c of the blocks (r, b): the quad-lane form computes its column locally and exchanges the Z's.
template <typename T>
OUZ_HD void pvf_g0(const M3T<T>& M, const T X0[3], const T X1[3], const T X2[3], T dt, T h, T out[3]) {
#pragma clang fp contract(off)
  T s[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k] = fma(dt, X1[k], h * X2[k]);
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = dot3s(M.m[i * 3], M.m[i * 3 + 1], M.m[i * 3 + 2], s[0], s[1], s[2], X0[i]);
}
template <typename T>
OUZ_HD void pvf_g1(const M3T<T>& M, const T X1[3], const T X2[3], T dt, T out[3]) {
#pragma clang fp contract(off)
  T s[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k] = fma(dt, X2[k], X1[k]);
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = dot3(M.m[i * 3], M.m[i * 3 + 1], M.m[i * 3 + 2], s[0], s[1], s[2]);
}
// column c of Z00, Z01, Z11 from column c of G_{0,1}, G_{0,2}, G_{1,1}, G_{1,2}
template <typename T>
OUZ_HD void pvf_z(const T g01[3], const T g02[3], const T g11[3], const T g12[3], T dt, T h, T z00[3], T z01[3],
                  T z11[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    z00[i] = fma(dt, g01[i], h * g02[i]);
    z01[i] = fma(dt, g02[i], g01[i]);
    z11[i] = fma(dt, g12[i], g11[i]);
  }
}

// prediction_step, covariance part only (the split form's covariance wave: quad_kernels.hip SplitPv)
template <typename T>
OUZ_HD void pv_cov_predict_t(T P[45], const M3T<T>& M, T dt) {
  const T h = dt * dt * T(0.5);
  const T q_a = (T)kPvAccVar, qhh = q_a * h * h, qhd = q_a * h * dt, qdd = q_a * dt * dt;
  // every G column from the old P before anything is written: g[b][c][i] = G_{0,b}[i][c], g1[b-1][c][i] = G_{1,b}
  T g0[3][3][3], g1[2][3][3];
#pragma unroll
  for (int b = 0; b < 3; ++b)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      T X0[3], X1[3], X2[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        X0[k] = P[s9(k, 3 * b + c)];
        X1[k] = P[s9(3 + k, 3 * b + c)];
        X2[k] = P[s9(6 + k, 3 * b + c)];
      }
      pvf_g0(M, X0, X1, X2, dt, h, g0[b][c]);
      if (b > 0) pvf_g1(M, X1, X2, dt, g1[b - 1][c]);
    }
  T z00[3][3], z01[3][3], z11[3][3];   // [column][row]
#pragma unroll
  for (int c = 0; c < 3; ++c) pvf_z(g0[1][c], g0[2][c], g1[0][c], g1[1][c], dt, h, z00[c], z01[c], z11[c]);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const T m0 = M.m[c * 3], m1 = M.m[c * 3 + 1], m2 = M.m[c * 3 + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (i <= c) P[s9(i, c)] = dot3s(z00[0][i], z00[1][i], z00[2][i], m0, m1, m2, i == c ? g0[0][c][i] + qhh : g0[0][c][i]);
      P[s9(i, 3 + c)] = dot3s(z01[0][i], z01[1][i], z01[2][i], m0, m1, m2, i == c ? qhd : T(0));
      if (i <= c) P[s9(3 + i, 3 + c)] = dot3s(z11[0][i], z11[1][i], z11[2][i], m0, m1, m2, i == c ? qdd : T(0));
      P[s9(i, 6 + c)] = g0[2][c][i];
      P[s9(3 + i, 6 + c)] = g1[1][c][i];
    }
  }
}

template <typename T>
OUZ_HD void pv_predict_t(T x[9], T P[45], const T acc[3], EkfQ q, T dt) {
  const M3T<T> M = pv_rot<T>(q);
  const T h = dt * dt * T(0.5);
  pv_state_predict(x, acc, M, dt, h);
  pv_cov_predict_t(P, M, dt);
}

// correction_step for one measured block m (0 = position, 1 = velocity) with R = r I.
// Stable form of x += K (z - x_m); P = (I - K H) P  (DESIGN.md §4), the other blocks A < B:
//   S = P_mm + r I;  K_o = P_om S^-1;  x_m = z - r S^-1 y;  x_o += K_o y   (y = z - x_m)
//   P_oo' = P_oo' - K_o P_mo';  P_mo = r K_o^T;  P_mm = r (I - r S^-1)
// R0 = true: the velocity fix as the reference runs it, R = 0 (PVFilter.py:76-79 tests gps_var): x_m = z and
// P_mm = P_mo = 0, written as zeros (IEEE f64 cannot fold 0 * x).
// Row i of K_o = row i of P_om times S^-1; element (i, c) of an updated block = seed - (row i of K) . (column c
// of P_mo); the quad-lane form computes row c of each K and column c of each block.
// The correction in three parts, each element by the same formula wherever it is evaluated: the gains from
// the covariance, the state update from the gains, the covariance update from the gains.
template <int MB, typename T>
OUZ_HD void pv_gain_t(const T P[45], T r, M3T<T>& Si, T KA[3][3], T KB[3][3]) {
#pragma clang fp contract(off)
  constexpr int A = (MB == 0) ? 1 : 0;   // the two other blocks, A < B
  constexpr int B = 2;
  M3T<T> S;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) S.m[i * 3 + j] = P[s9(3 * MB + i, 3 * MB + j)];
  S.m[0] += r; S.m[4] += r; S.m[8] += r;
  Si = inv_sym3(S);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      KA[i][j] = dot3(P[s9(3 * A + i, 3 * MB)], P[s9(3 * A + i, 3 * MB + 1)], P[s9(3 * A + i, 3 * MB + 2)],
                      Si.m[j], Si.m[3 + j], Si.m[6 + j]);
      KB[i][j] = dot3(P[s9(3 * B + i, 3 * MB)], P[s9(3 * B + i, 3 * MB + 1)], P[s9(3 * B + i, 3 * MB + 2)],
                      Si.m[j], Si.m[3 + j], Si.m[6 + j]);
    }
}

template <int MB, typename T, bool R0 = false>
OUZ_HD void pv_x_correct_t(T x[9], const T z[3], T r, const M3T<T>& Si, const T KA[3][3], const T KB[3][3]) {
#pragma clang fp contract(off)
  constexpr int A = (MB == 0) ? 1 : 0;
  constexpr int B = 2;
  T y[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) y[k] = z[k] - x[MB * 3 + k];
  T xm[3], dA[3], dB[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    xm[i] = R0 ? z[i] : fma(-r, dot3(Si.m[i * 3], Si.m[i * 3 + 1], Si.m[i * 3 + 2], y[0], y[1], y[2]), z[i]);
    dA[i] = dot3(KA[i][0], KA[i][1], KA[i][2], y[0], y[1], y[2]);
    dB[i] = dot3(KB[i][0], KB[i][1], KB[i][2], y[0], y[1], y[2]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    x[MB * 3 + k] = xm[k];
    x[A * 3 + k] += dA[k];
    x[B * 3 + k] += dB[k];
  }
}

template <int MB, typename T, bool R0 = false>
OUZ_HD void pv_cov_correct_t(T P[45], T r, const M3T<T>& Si, const T KA[3][3], const T KB[3][3]) {
#pragma clang fp contract(off)
  constexpr int A = (MB == 0) ? 1 : 0;
  constexpr int B = 2;
  // the other-other blocks first: they read the m-row blocks, which are overwritten below
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const T pb0 = P[s9(3 * MB, 6 + c)], pb1 = P[s9(3 * MB + 1, 6 + c)], pb2 = P[s9(3 * MB + 2, 6 + c)];
    const T pa0 = P[s9(3 * MB, 3 * A + c)], pa1 = P[s9(3 * MB + 1, 3 * A + c)], pa2 = P[s9(3 * MB + 2, 3 * A + c)];
    T bb[3], ab[3], aa[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      bb[i] = dot3s(-KB[i][0], -KB[i][1], -KB[i][2], pb0, pb1, pb2, P[s9(6 + i, 6 + c)]);
      ab[i] = dot3s(-KA[i][0], -KA[i][1], -KA[i][2], pb0, pb1, pb2, P[s9(3 * A + i, 6 + c)]);
      aa[i] = dot3s(-KA[i][0], -KA[i][1], -KA[i][2], pa0, pa1, pa2, P[s9(3 * A + i, 3 * A + c)]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (i <= c) P[s9(6 + i, 6 + c)] = bb[i];
      P[s9(3 * A + i, 6 + c)] = ab[i];
      if (i <= c) P[s9(3 * A + i, 3 * A + c)] = aa[i];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if constexpr (R0) {
        if (MB < A) P[s9(3 * MB + i, 3 * A + c)] = T(0); else P[s9(3 * A + i, 3 * MB + c)] = T(0);
        P[s9(3 * MB + i, 6 + c)] = T(0);
        if (i <= c) P[s9(3 * MB + i, 3 * MB + c)] = T(0);
      } else {
        if (MB < A) P[s9(3 * MB + i, 3 * A + c)] = r * KA[c][i]; else P[s9(3 * A + i, 3 * MB + c)] = r * KA[i][c];
        P[s9(3 * MB + i, 6 + c)] = r * KB[c][i];
        if (i <= c) P[s9(3 * MB + i, 3 * MB + c)] = r * fma(-r, Si.m[i * 3 + c], i == c ? T(1) : T(0));
      }
    }
}

template <int MB, typename T, bool R0 = false>
OUZ_HD void pv_correct_t(T x[9], T P[45], const T z[3], T r) {
  M3T<T> Si;
  T KA[3][3], KB[3][3];
  pv_gain_t<MB, T>(P, r, Si, KA, KB);
  pv_x_correct_t<MB, T, R0>(x, z, r, Si, KA, KB);
  pv_cov_correct_t<MB, T, R0>(P, r, Si, KA, KB);
}

// One PV-filter step as the driver runs it (ekf_lee_landed.py:417-444): predict, then the
// position fix if triggered, then the velocity fix (R = 0) if triggered.  The state and
// covariance are STORED in f32 but the whole step is evaluated in PvReal: the covariance
// carries ~10 decades between the R = 1e-7 fixed position and the O(1e3) bias directions,
// and rounding it to f32 between predict and correct loses the bias information
// (the reference's own f32 evaluation drifts by ~2x the state).
typedef double PvReal;

OUZ_HD void pv_step(float xf[9], float Pf[45], V3 acc, EkfQ q, float dt, bool pos_fix, V3 zp, bool vel_fix, V3 zv) {
  PvReal x[9], P[45];
#pragma unroll
  for (int k = 0; k < 9; ++k) x[k] = (PvReal)xf[k];
#pragma unroll
  for (int k = 0; k < 45; ++k) P[k] = (PvReal)Pf[k];
  const PvReal a[3] = {(PvReal)acc.x, (PvReal)acc.y, (PvReal)acc.z};
  pv_predict_t<PvReal>(x, P, a, q, (PvReal)dt);
  if (pos_fix) {
    const PvReal z[3] = {(PvReal)zp.x, (PvReal)zp.y, (PvReal)zp.z};
    pv_correct_t<0, PvReal>(x, P, z, (PvReal)kPvPosVar);
  }
  if (vel_fix) {
    const PvReal z[3] = {(PvReal)zv.x, (PvReal)zv.y, (PvReal)zv.z};
    pv_correct_t<1, PvReal, true>(x, P, z, PvReal(0));
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) xf[k] = (float)x[k];
#pragma unroll
  for (int k = 0; k < 45; ++k) Pf[k] = (float)P[k];
}

// Single-call forms (PVFilter.prediction_step / correction_step) on f32 storage.
OUZ_HD void pv_predict(float xf[9], float Pf[45], V3 acc, EkfQ q, float dt) {
  pv_step(xf, Pf, acc, q, dt, false, acc, false, acc);
}
template <int MB>
OUZ_HD void pv_correct(float xf[9], float Pf[45], V3 z, float r) {
  PvReal x[9], P[45];
#pragma unroll
  for (int k = 0; k < 9; ++k) x[k] = (PvReal)xf[k];
#pragma unroll
  for (int k = 0; k < 45; ++k) P[k] = (PvReal)Pf[k];
  const PvReal zz[3] = {(PvReal)z.x, (PvReal)z.y, (PvReal)z.z};
  pv_correct_t<MB, PvReal>(x, P, zz, (PvReal)r);
#pragma unroll
  for (int k = 0; k < 9; ++k) xf[k] = (float)x[k];
#pragma unroll
  for (int k = 0; k < 45; ++k) Pf[k] = (float)P[k];
}

// ---------------------------------------------------------------------------
// Reward / observation
// ---------------------------------------------------------------------------
// compute_ingenuity_reward (tasks/ekf_lee_landed.py:692-723).
// distance to the target: the reward's position term and the die test (one formula for both)
OUZ_HD float target_dist(V3 p, V3 target) {
  V3 d = target - p;
  return sqrtf(dot(d, d));
}

OUZ_HD float reward(V3 p, V3 target, Q4 q, V3 w, float& dist) {
  dist = target_dist(p, target);
  float pos_r = 1.0f / (1.0f + dist * dist);
  float ups_z = 2.0f * q.w * q.w - 1.0f + q.z * q.z * 2.0f;      // quat_axis(q, 2).z
  float tilt = fabsf(1.0f - ups_z);
  float up_r = 5.0f / (1.0f + tilt * tilt);
  float spin = fabsf(w.z);
  float spin_r = 1.0f / (1.0f + spin * spin);
  return pos_r + pos_r * (up_r + spin_r);
}

// ---------------------------------------------------------------------------
// Lumped rigid-body integrator (build-defined; PhysX is closed — DESIGN.md §3)
// ---------------------------------------------------------------------------
constexpr float kGravity = 9.81f;

// f_b / tau_b: body-frame force and torque at the COM (LOCAL_SPACE, ekf_lee_landed.py:525);
// inv_I = 1/I (diagonal).  Semi-implicit Euler; exact exponential map for the attitude.
// Landing deck of the husky (build-defined contact; oracle deck_contact): the drone
// root rests at z 0.375 (the reference's recorded landings), footprint = the disk inscribed in the
// 0.5709 m wide chassis (husky.urdf:61-69).  Inelastic, sticking: on the deck the drone moves with
// the platform and stops rotating.
constexpr float kDeckZRest = 0.375f;
constexpr float kDeckRadius2 = (0.5709f * 0.5f) * (0.5709f * 0.5f);
struct DeckContact {
  bool on;
  float px, py, vx, vy;   // platform position / velocity (xy)
};

// kThrustOnly: f_b = (0, 0, f_b.z) (every task's rotor force is along body z); the world force is then
// R's third column times f_b.z, the same value mv(R, f_b) rounds to without its multiplies by zero.
template <bool kThrustOnly = false>
OUZ_HD void integrate(V3& p, Q4& q, V3& v, V3& w, V3 f_b, V3 tau_b, float inv_m, V3 I, V3 inv_I, float dt,
                      int substeps, float wmax, DeckContact deck = DeckContact{false, 0.f, 0.f, 0.f, 0.f}) {
  const float h = dt / (float)substeps;
  for (int s = 0; s < substeps; ++s) {
    M3 R = quat_to_mat(q);
    V3 fw = kThrustOnly ? v3(R.m[2] * f_b.z, R.m[5] * f_b.z, R.m[8] * f_b.z) : mv(R, f_b);
    v = v + h * v3(fw.x * inv_m, fw.y * inv_m, fw.z * inv_m - kGravity);
    V3 wb = mtv(R, w);
    V3 c = cross(wb, mul(I, wb));
    wb = wb + h * mul(inv_I, tau_b - c);
    w = mv(R, wb);
    float n2 = dot(w, w);
    if (n2 > wmax * wmax) w = (wmax / sqrtf(n2)) * w;
    p = p + h * v;
    if (deck.on) {
      const float dx = p.x - deck.px, dy = p.y - deck.py;
      if (dx * dx + dy * dy < kDeckRadius2 && p.z < kDeckZRest) {
        p.z = kDeckZRest;
        v = v3(deck.vx, deck.vy, fmaxf(v.z, 0.0f));
        w = v3(0.0f, 0.0f, 0.0f);
      }
    }
    // dq = [sin(th) w/|w|, cos(th)], th = |w| h / 2.  |w| <= wmax keeps th small at the
    // configured dt (4 pi * 0.005 / 2 = 0.031 rad): there the Taylor series to th^5 / th^6
    // is exact in f32 and replaces the libm sin/cos.
    float n = sqrtf(dot(w, w));
    float th = 0.5f * h * n, th2 = th * th;
    float sc, co;
    if (th < 0.1f) {
      sc = 0.5f * h * (1.0f - th2 * (1.0f / 6.0f) * (1.0f - th2 * (1.0f / 20.0f)));        // sin(th)/|w|
      co = 1.0f - 0.5f * th2 * (1.0f - th2 * (1.0f / 12.0f) * (1.0f - th2 * (1.0f / 30.0f)));
    } else {
      sc = sinf(th) / n;
      co = cosf(th);
    }
    Q4 dq{w.x * sc, w.y * sc, w.z * sc, co};
    q = quat_mul(dq, q);
    float qi = 1.0f / sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    q = Q4{q.x * qi, q.y * qi, q.z * qi, q.w * qi};
  }
}

// The same integrator specialised for the fused step (every task's body force is a thrust along
// body z) with the angular velocity carried in the body frame across sub-steps.  The attitude
// increment of a sub-step rotates about w itself (dq = exp(w h / 2) ⊗ q), so R_{s+1}^T w = R_s^T w:
// the body rate after sub-step s is the next sub-step's input without the world -> body -> world
// round trip, and dq ⊗ q = q ⊗ exp(w_b h / 2).  Algebraically identical to integrate<true>
// (the oracle keeps the world-frame form); it needs R(q) once at entry (shared with the
// controller), R(q)'s third column between sub-steps and R(q) once at exit for the world-frame w.
// |w| = |w_b| (the clamp) and w = 0 <=> w_b = 0 (the deck) carry over unchanged.
// NSUB > 0: that many sub-steps, unrolled; NSUB = 0: nsub sub-steps in a loop.  g: the gravity vector.
// R_out (optional): receives R(q) of the post-step quaternion, formed here for the world-frame body rate (the fused
// rollout hands it to its next step as R0).
// SMALL: the launch guarantees 0.5 h wmax < 0.04 with margin (plain_config, quad_env.h): |w_b| <= wmax after the clamp
// (or 0 on the deck), so every sub-step takes the series side of the angle test and that side is the only code.
// RARE_CLAMP: the caller's lanes are seldom above the body-rate clamp (the plain LeeLanded rollout: a controlled
// hover); the clamp is then laid out of line and a sub-step without it falls through.  Not for the RL tasks, whose
// random-action lanes sit at the clamp in most steps (QuadFault 8192 envs: -4.7 % env-steps/s with the hint).
template <int NSUB, bool SMALL = false, bool RARE_CLAMP = false>
OUZ_HD void integrate_thrust_body(V3& p, Q4& q, V3& v, V3& w, const M3& R0, float fz, V3 tau_b, float inv_m, V3 I,
                                  V3 inv_I, float h, float wmax, DeckContact deck, V3 g, int nsub = NSUB,
                                  M3* R_out = nullptr) {
  V3 wb = mtv(R0, w);
  V3 z = v3(R0.m[2], R0.m[5], R0.m[8]);
  const float acc = fz * inv_m;
  for (int s = 0; s < (NSUB > 0 ? NSUB : nsub); ++s) {   // a constant NSUB unrolls by itself
    // probe build: the boundary between the plain kernels' two sub-steps (slot 5 is the estimator's otherwise)
    if (SMALL && s == 1) OUZ_SUBSTEP_STAMP(5);
    if (s > 0)   // third column of R(q) for the unit quaternion q (normalised at the end of every sub-step)
      z = v3(2.0f * (q.x * q.z + q.y * q.w), 2.0f * (q.y * q.z - q.x * q.w), 1.0f - 2.0f * (q.x * q.x + q.y * q.y));
    // g: the sim's gravity, (0, 0, -kGravity) unless sim_params DR'd (with g.x = g.y = 0 the x / y terms round as
    // the plain products: a * b + 0 is the product)
    v = v + h * v3(z.x * acc + g.x, z.y * acc + g.y, z.z * acc + g.z);
    const V3 c = cross(wb, mul(I, wb));
    wb = wb + h * mul(inv_I, tau_b - c);
    float n2 = dot(wb, wb);
    const bool over = n2 > wmax * wmax;
    if (RARE_CLAMP ? __builtin_expect(over, 0) : over) { wb = (wmax / sqrtf(n2)) * wb; n2 = wmax * wmax; }
    p = p + h * v;
    if (deck.on) {
      const float dx = p.x - deck.px, dy = p.y - deck.py;
      if (dx * dx + dy * dy < kDeckRadius2 && p.z < kDeckZRest) {
        p.z = kDeckZRest;
        v = v3(deck.vx, deck.vy, fmaxf(v.z, 0.0f));
        wb = v3(0.0f, 0.0f, 0.0f);
        n2 = 0.0f;
      }
    }
    const float n = sqrtf(n2);
    const float th = 0.5f * h * n, th2 = th * th;
    float sc, co;
    if (SMALL || th < 0.04f) {
      // |w| <= 4 pi at the configured dt keeps th <= 0.0315: the series to th^2 (sin) / th^4 (cos) is
      // exact in f32 there (the next terms are < 1e-8 relative)
      sc = 0.5f * h * (1.0f - th2 * (1.0f / 6.0f));
      co = 1.0f - 0.5f * th2 * (1.0f - th2 * (1.0f / 12.0f));
    } else {   // only at other dt / sub-step settings (th <= h |w|max / 2): small arguments, no range reduction
      sc = __sinf(th) / n;
      co = __cosf(th);
    }
    q = quat_mul(q, Q4{wb.x * sc, wb.y * sc, wb.z * sc, co});
    // renormalise once, after the last sub-step: a product of unit quaternions stays unit to a few
    // ulp, which the next sub-step's third-column formula tolerates
    const bool last = NSUB > 0 ? s == NSUB - 1 : s == nsub - 1;
    if (last) {
      const float qi = 1.0f / sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
      q = Q4{q.x * qi, q.y * qi, q.z * qi, q.w * qi};
    }
  }
  const M3 R1 = quat_to_mat(q);
  w = mv(R1, wb);
  if (R_out) *R_out = R1;
}

#ifndef OUZ_HOST
// ---------------------------------------------------------------------------
// Packed-pair forms (device only; DESIGN.md §5.1, docs/HISTORY.md round 20)
// ---------------------------------------------------------------------------
// The plain LeeLanded rollout's state wave runs alone on its SIMD and is bound by its instruction count; a
// v_pk_{mul,add,fma}_f32 does two f32 operations in one issue slot of that wave.  Here the 3-vector math of its
// chain is laid out once as (x, y) pairs plus a scalar z, so that the element-wise work, the matrix-vector products
// and Rd^T R go through packed instructions without re-pairing registers between them.
// The rule that keeps the bits: every half of every packed operation is the scalar form's operation on the same
// operands, and every expression below has the shape of the scalar source's (a * b + c inside one expression fuses
// in both, a product stored and added later in neither).  Dot products, norms and cross products stay scalar: a dot
// is one chain, and a cross needs the (y, z, x) rotation, which no aligned register pair holds.
#define OUZ_PK __device__ __forceinline__
typedef float F2 __attribute__((ext_vector_type(2)));
struct P3 { F2 xy; float z; };
struct PQ { F2 xy, zw; };                  // xyzw
// R(q) by rows (r_i = (m[3i], m[3i+1]), m[3i+2]: what mtv and Rd^T R read) and by columns (c_j = (m[j], m[3+j]),
// m[6+j]: what mv reads; c2 is the body z axis).  Each element is computed once; a consumer takes what it reads.
struct PR { P3 r0, r1, r2, c0, c1, c2; };

OUZ_PK P3 p3(V3 a) { return P3{F2{a.x, a.y}, a.z}; }
OUZ_PK V3 v3(P3 a) { return V3{a.xy.x, a.xy.y, a.z}; }
OUZ_PK PQ pq(Q4 a) { return PQ{F2{a.x, a.y}, F2{a.z, a.w}}; }
OUZ_PK Q4 q4(PQ a) { return Q4{a.xy.x, a.xy.y, a.zw.x, a.zw.y}; }
OUZ_PK P3 operator+(P3 a, P3 b) { return P3{a.xy + b.xy, a.z + b.z}; }
OUZ_PK P3 operator-(P3 a, P3 b) { return P3{a.xy - b.xy, a.z - b.z}; }
OUZ_PK P3 operator*(float s, P3 a) { return P3{s * a.xy, s * a.z}; }
OUZ_PK P3 mul(P3 a, P3 b) { return P3{a.xy * b.xy, a.z * b.z}; }
OUZ_PK float dot(P3 a, P3 b) { return a.xy.x * b.xy.x + a.xy.y * b.xy.y + a.z * b.z; }
OUZ_PK float norm(P3 a) { return sqrtf(dot(a, a)); }
OUZ_PK P3 cross(P3 a, P3 b) {
  const float ax = a.xy.x, ay = a.xy.y, bx = b.xy.x, by = b.xy.y;
  return P3{F2{ay * b.z - a.z * by, a.z * bx - ax * b.z}, ax * by - ay * bx};
}
// a v.x + b v.y + c v.z: mtv(A, v) of A's rows a, b, c; mv(A, v) of A's columns a, b, c
OUZ_PK P3 lin3(P3 a, P3 b, P3 c, P3 v) {
  const float vx = v.xy.x, vy = v.xy.y;
  return P3{a.xy * vx + b.xy * vy + c.xy * v.z, a.z * vx + b.z * vy + c.z * v.z};
}
// v.x a + v.y b + v.z c: row i of Rd^T R from Rd's column i (v) and R's rows
OUZ_PK P3 lin3l(P3 v, P3 a, P3 b, P3 c) {
  const float vx = v.xy.x, vy = v.xy.y;
  return P3{vx * a.xy + vy * b.xy + v.z * c.xy, vx * a.z + vy * b.z + v.z * c.z};
}
OUZ_PK P3 mtv(const PR& A, P3 v) { return lin3(A.r0, A.r1, A.r2, v); }
OUZ_PK P3 mv(const PR& A, P3 v) { return lin3(A.c0, A.c1, A.c2, v); }

// One-instruction helpers where the compiler does not fold a half-negation into the operand modifiers (it negates
// the whole pair with a v_pk_add_f32 and blends the halves with moves).  Each is a fused multiply-add per half, as the
// scalar source's a * b + c and a * b - c inside one expression are; neg_lo / neg_hi flip a sign bit exactly.
// a b.x + (c.x, -c.y)
OUZ_PK F2 pk_fma_bx_nhi(F2 a, F2 b, F2 c) {
  F2 d;
  __asm__("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1] neg_hi:[0,0,1]" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
// a b.x + (-c.x, c.y)
OUZ_PK F2 pk_fma_bx_nlo(F2 a, F2 b, F2 c) {
  F2 d;
  __asm__("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1] neg_lo:[0,0,1]" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
// a.x a.y + (-c.x, c.x)
OUZ_PK F2 pk_fma_xy_ncx(F2 a, F2 c) {
  F2 d;
  __asm__("v_pk_fma_f32 %0, %1, %1, %2 op_sel:[0,1,0] op_sel_hi:[0,1,0] neg_lo:[0,0,1]" : "=v"(d) : "v"(a), "v"(c));
  return d;
}

// quat_to_mat: the off-diagonal pairs (m2, m5) and (m6, m7) share the products (j r, i r); (m1, m3) differ in the
// sign of k r; (m0, m4) share k k.
OUZ_PK PR quat_to_mat(PQ q) {
  const float r = q.zw.y, i = q.xy.x, j = q.xy.y, k = q.zw.x;
  const float two_s = 2.0f / (r * r + i * i + j * j + k * k);
  const F2 ji = q.xy.yx;
  const F2 t = ji * r;                                         // (j r, i r)
  const F2 krp = q.zw * q.zw.yx;                               // (k r, r k): one value
  const float kk = k * k;
  const F2 m04 = 1.0f - two_s * (ji * ji + kk);                // (j j + k k, i i + k k)
  const float m8 = 1.0f - two_s * (i * i + j * j);
  const F2 m13 = two_s * pk_fma_xy_ncx(q.xy, krp);             // (i j - k r, i j + k r)
  const F2 m25 = two_s * pk_fma_bx_nhi(q.xy, q.zw, t);         // (i k + j r, j k - i r)
  const F2 m67 = two_s * pk_fma_bx_nlo(q.xy, q.zw, t);         // (i k - j r, j k + i r)
  return PR{P3{F2{m04.x, m13.x}, m25.x}, P3{F2{m13.y, m04.y}, m25.y}, P3{m67, m8},
            P3{F2{m04.x, m13.y}, m67.x}, P3{F2{m13.x, m04.y}, m67.y}, P3{m25, m8}};
}
OUZ_PK PR pr(const M3& R) {
  return PR{P3{F2{R.m[0], R.m[1]}, R.m[2]}, P3{F2{R.m[3], R.m[4]}, R.m[5]}, P3{F2{R.m[6], R.m[7]}, R.m[8]},
            P3{F2{R.m[0], R.m[3]}, R.m[6]}, P3{F2{R.m[1], R.m[4]}, R.m[7]}, P3{F2{R.m[2], R.m[5]}, R.m[8]}};
}
OUZ_PK M3 m3(const PR& R) {
  return M3{{R.r0.xy.x, R.r0.xy.y, R.r0.z, R.r1.xy.x, R.r1.xy.y, R.r1.z, R.r2.xy.x, R.r2.xy.y, R.r2.z}};
}

// unit2 of two independent argument pairs, side by side: (s, c)[k] = unit2(y[k], x[k])
OUZ_PK void unit2(F2 y, F2 x, F2& s, F2& c) {
  const F2 h2 = x * x + y * y;
  const F2 ih{1.0f / sqrtf(h2.x), 1.0f / sqrtf(h2.y)};
  const F2 ys = y * ih, xc = x * ih;
  s = F2{h2.x > 0.0f ? ys.x : 0.0f, h2.y > 0.0f ? ys.y : 0.0f};
  c = F2{h2.x > 0.0f ? xc.x : 1.0f, h2.y > 0.0f ? xc.y : 1.0f};
}
OUZ_PK EulerSC euler_sc(const PR& R) {   // its two unit2 calls as one: (roll, yaw)
  EulerSC e;
  F2 s, c;
  unit2(F2{R.r2.xy.y, R.r1.xy.x}, F2{R.r2.z, R.r0.xy.x}, s, c);
  e.sr = s.x; e.cr = c.x;
  e.sp = -R.r2.xy.x;
  e.cp = sqrtf(fmaxf(0.0f, 1.0f - R.r2.xy.x * R.r2.xy.x));
  e.sy = s.y; e.cy = c.y;
  return e;
}

OUZ_PK PQ quat_mul(PQ a, PQ b) {
  const float ax = a.xy.x, ay = a.xy.y, az = a.zw.x, aw = a.zw.y, bx = b.xy.x, by = b.xy.y, bz = b.zw.x, bw = b.zw.y;
  const F2 cxy{ay * bz - az * by, az * bx - ax * bz};
  return PQ{aw * b.xy + bw * a.xy + cxy, F2{aw * bz + bw * az + (ax * by - ay * bx), aw * bw - (ax * bx + ay * by + az * bz)}};
}

// third column of R(q) for the unit quaternion q (the integrator's, between sub-steps)
OUZ_PK P3 third_col(PQ q) {
  const F2 t = q.xy.yx * q.zw.y;   // (q.y q.w, q.x q.w)
  return P3{2.0f * pk_fma_bx_nhi(q.xy, q.zw, t), 1.0f - 2.0f * (q.xy.x * q.xy.x + q.xy.y * q.xy.y)};   // q.xy q.z + (t.x, -t.y)
}
OUZ_PK PQ normalise(PQ q) {
  const float qi = 1.0f / sqrtf(q.xy.x * q.xy.x + q.xy.y * q.xy.y + q.zw.x * q.zw.x + q.zw.y * q.zw.y);
  return PQ{q.xy * qi, q.zw * qi};
}

struct LeeGainsP { P3 kP, kV, kR, kW; };
OUZ_PK LeeGainsP gains_p(const LeeGains& g) { return LeeGainsP{p3(g.kP), p3(g.kV), p3(g.kR), p3(g.kW)}; }

// lee_attitude_loop with Rd given by its columns b1, b2, b3
OUZ_PK P3 lee_attitude_loop(const PR& R, P3 b1, P3 b2, P3 b3, P3 omega, const EulerSC& e, float yaw_rate,
                             const LeeGainsP& g) {
  const P3 A0 = lin3l(b1, R.r0, R.r1, R.r2), A1 = lin3l(b2, R.r0, R.r1, R.r2), A2 = lin3l(b3, R.r0, R.r1, R.r2);   // rows of Rd^T R
  const P3 e_R{F2{0.5f * (A2.xy.y - A1.z), 0.5f * (A0.z - A2.xy.x)}, 0.5f * (A1.xy.x - A0.xy.y)};
  const P3 wd{F2{-e.sp * yaw_rate, e.sr * e.cp * yaw_rate}, e.cr * e.cp * yaw_rate};
  const P3 des = lin3(A0, A1, A2, wd);
  const P3 act = mtv(R, omega);
  const P3 e_w = act - des;
  return P3{-g.kR.xy * e_R.xy - g.kW.xy * e_w.xy, -g.kR.z * e_R.z - g.kW.z * e_w.z};
}

// lee_position_R<true> for a command on the z axis, (0, 0, cmd_z), which is the plain LeeLanded rollout's hover point.
// The x / y position error is written -p: the scalar build selects the 0 - p.x that feeds the gain's multiply as a
// negated operand of that multiply (so p.x = +0 gives -0 there, not the subtraction's +0), and the packed build would
// keep the subtraction; written as the negation, both evaluate (-p.x) kP.x.
OUZ_PK void lee_position_R(const PR& R, P3 p, P3 v, P3 w, float cmd_z, const LeeGainsP& g, float& thrust, P3& torque) {
  const EulerSC e = euler_sc(R);
  P3 a = mul(g.kP, P3{-p.xy, cmd_z - p.z}) - mul(g.kV, v);
  a.z += 1.0f;
  thrust = a.xy.x * R.c2.xy.x + a.xy.y * R.c2.xy.y + a.z * R.c2.z;
  const P3 b3 = (1.0f / norm(a)) * a;
  P3 b2 = cross(b3, P3{F2{e.cy, e.sy}, 0.0f});
  b2 = (1.0f / norm(b2)) * b2;
  const P3 b1 = cross(b2, b3);
  const float ya = 0.0f - atan2_bounded_f(R.r1.xy.x, R.r0.xy.x);
  float yr = remainder_small_f(ya, kTwoPiF);
  if (yr > kPiF) yr -= kTwoPiF;
  torque = lee_attitude_loop(R, b1, b2, b3, w, e, yr, g);
}

// integrate_thrust_body<2, true, RARE_CLAMP> with its R_out
template <bool RARE_CLAMP>
OUZ_PK void integrate_thrust_body2(P3& p, PQ& q, P3& v, P3& w, const PR& R0, float fz, P3 tau_b, float inv_m, P3 I,
                                    P3 inv_I, float h, float wmax, DeckContact deck, P3 g, PR& R_out) {
  P3 wb = mtv(R0, w);
  P3 z = R0.c2;
  const float acc = fz * inv_m;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (s == 1) OUZ_SUBSTEP_STAMP(5);
    if (s > 0) z = third_col(q);
    v = v + h * P3{z.xy * acc + g.xy, z.z * acc + g.z};
    const P3 c = cross(wb, mul(I, wb));
    wb = wb + h * mul(inv_I, tau_b - c);
    float n2 = dot(wb, wb);
    const bool over = n2 > wmax * wmax;
    if (RARE_CLAMP ? __builtin_expect(over, 0) : over) { wb = (wmax / sqrtf(n2)) * wb; n2 = wmax * wmax; }
    p = p + h * v;
    if (deck.on) {
      const F2 d = p.xy - F2{deck.px, deck.py};
      if (d.x * d.x + d.y * d.y < kDeckRadius2 && p.z < kDeckZRest) {
        p.z = kDeckZRest;
        v = P3{F2{deck.vx, deck.vy}, fmaxf(v.z, 0.0f)};
        wb = P3{F2{0.0f, 0.0f}, 0.0f};
        n2 = 0.0f;
      }
    }
    const float n = sqrtf(n2);
    const float th = 0.5f * h * n, th2 = th * th;
    const float sc = 0.5f * h * (1.0f - th2 * (1.0f / 6.0f));
    const float co = 1.0f - 0.5f * th2 * (1.0f - th2 * (1.0f / 12.0f));
    q = quat_mul(q, PQ{wb.xy * sc, F2{wb.z * sc, co}});
    if (s == 1) q = normalise(q);   // once, after the last sub-step
  }
  R_out = quat_to_mat(q);
  w = mv(R_out, wb);
}
#endif  // !OUZ_HOST

}  // namespace ouz
