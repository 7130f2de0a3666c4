// Calibration records (definition: include/spe.h spe_calibration_records): per image the pose error
// against ground truth in the covariance's own perturbation convention, its NEES under the predicted
// covariance, and per landmark the keypoint error in units of the predicted sigma.  What a calibration
// of the sigmas is accumulated from (spe/calibration.py); nothing here feeds back into a solver.
//
// One wave per image, CAL_WAVES images per work-group, like pose_cov_kernel; no LDS, no barrier, no
// atomics (the waves of a group share nothing).  Lane q takes query q's label and score; lane l < C - 1
// then owns landmark l: it finds the landmark's query by the selection's rule over the wave's (label,
// score) pairs -- argmax_class / takes_over of pnp_math.h, the code the solver, spe_self_assess and
// spe_pose_covariance run -- projects the ground-truth point and writes its z-score and flags.  Lane 0
// forms the pose error and the three Cholesky solves.  Compiled with -ffp-contract=off like pnp.hip:
// every fp64 step rounds on its own, as the numpy restatement's does.
#include "spe_common.h"
#include "pnp_math.h"
#include "spe_pnp.h"

namespace {

constexpr int WAVE = 64;
constexpr int CAL_WAVES = 4;

SPE_DEV bool finite_d(double x) { return fabs(x) < (double)INFINITY; }

// d^T S^-1 d for the symmetric 6x6 S (row-major, both triangles), by Cholesky of the Jacobi-scaled
// matrix; false when a diagonal is not positive and finite or a pivot is <= 64 eps
SPE_DEV bool nees6(const double* S, const double* d, double* out) {
  double s[6], A[36], L[6][6], b[6], x[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double v = S[i * 7];
    if (!(v > 0) || !finite_d(v)) return false;
    s[i] = 1.0 / sqrt(v);
  }
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) A[i * 6 + j] = (S[i * 6 + j] * s[i]) * s[j];
  if (!chol6_factor(A, 64.0 * DBL_EPSILON, L)) return false;
#pragma unroll
  for (int i = 0; i < 6; ++i) b[i] = d[i] * s[i];
  chol6_backsolve(L, b, x);
  double r = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) r += b[i] * x[i];
  *out = r;
  return true;
}

// the same for the 3x3 diagonal block of S that starts at row / column o
SPE_DEV bool nees3(const double* S, int o, const double* d, double* out) {
  double s[3], A[9], L[3][3], b[3], x[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double v = S[(o + i) * 7];
    if (!(v > 0) || !finite_d(v)) return false;
    s[i] = 1.0 / sqrt(v);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) A[i * 3 + j] = (S[(o + i) * 6 + o + j] * s[i]) * s[j];
  if (!chol3_factor(A, 64.0 * DBL_EPSILON, L)) return false;
#pragma unroll
  for (int i = 0; i < 3; ++i) b[i] = d[i] * s[i];
  chol3_backsolve(L, b, x);
  *out = b[0] * x[0] + b[1] * x[1] + b[2] * x[2];
  return true;
}

__global__ __launch_bounds__(WAVE * CAL_WAVES) void calib_records_kernel(CalibArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int b = blockIdx.x * CAL_WAVES + (int)(threadIdx.x / WAVE);
  if (b >= a.B) return;                               // wave-uniform
  const int Q = a.Q, C = a.C, Lm = C - 1;

  // ground truth (every lane, uniform): the unit quaternion's rotation, the inverse of blender_quat
  double qg[4], tg[3];
  double n2 = 0;
  for (int i = 0; i < 4; ++i) { qg[i] = a.q_gt[4 * b + i]; n2 += qg[i] * qg[i]; }
  for (int i = 0; i < 3; ++i) tg[i] = a.t_gt[3 * b + i];
  const double qn = sqrt(n2);
  const bool gt_ok = qn > 0 && finite_d(qn) && finite_d(tg[0]) && finite_d(tg[1]) && finite_d(tg[2]);
  if (!gt_ok) {
    if (lane < Lm) {
      a.z[((size_t)b * Lm + lane) * 2] = 0.0;
      a.z[((size_t)b * Lm + lane) * 2 + 1] = 0.0;
      a.kp_flags[(size_t)b * Lm + lane] = 0;
    }
    if (lane == 0) {
      for (int i = 0; i < 6; ++i) a.delta[6 * b + i] = 0.0;
      for (int i = 0; i < 3; ++i) a.nees[3 * b + i] = 0.0;
      a.calib_status[b] = 1;
    }
    return;
  }
  for (int i = 0; i < 4; ++i) qg[i] = qg[i] / qn;
  const double w = qg[0], x = qg[1], y = qg[2], z = qg[3];
  const double Rg[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};

  // selection, as in pose_cov_kernel
  int lab_q = C - 1;
  float sc_q = 0.f;
  if (lane < Q) lab_q = argmax_class(a.probs + ((size_t)b * Q + lane) * C, C, &sc_q);
  const int st = a.status[b];
  const bool have_pose = st == SPE_PNP_OK || st == SPE_PNP_RANSAC_FALLBACK;
  const uint32_t inl = have_pose ? a.inlier_mask[b] : 0u;
  const int mylab = lane < Lm ? lane : -1;
  int best_q = -1;
  float best_s = 0.f;
  for (int q = 0; q < Q; ++q) {
    const int l = __shfl(lab_q, q);
    const float s = __shfl(sc_q, q);
    if (l == mylab && takes_over(best_q, best_s, s)) { best_q = q; best_s = s; }
  }

  if (lane < Lm) {
    bool inlier = false;
    for (int i = 0; i < MAXN; ++i)
      if (((inl >> i) & 1u) && a.corr_label[MAXN * b + i] == mylab) inlier = true;
    inlier = inlier && best_q >= 0;
    double zx = 0, zy = 0;
    bool valid = false;
    if (best_q >= 0) {
      const double* X = a.world + 3 * mylab;
      const double xc = (Rg[0] * X[0] + Rg[1] * X[1] + Rg[2] * X[2]) + tg[0];
      const double yc = (Rg[3] * X[0] + Rg[4] * X[1] + Rg[5] * X[2]) + tg[1];
      const double zc = (Rg[6] * X[0] + Rg[7] * X[1] + Rg[8] * X[2]) + tg[2];
      const float* pt = a.points + ((size_t)b * Q + best_q) * 2;
      const float* sg = a.sigmas + ((size_t)b * Q + best_q) * 2;
      const double px = (double)pt[0], py = (double)pt[1];
      double sx = (double)sg[0], sy = (double)sg[1];
      if (a.sigma_scale) { sx *= (double)a.sigma_scale[2 * b]; sy *= (double)a.sigma_scale[2 * b + 1]; }
      sx *= a.sigma_gain;
      sy *= a.sigma_gain;
      valid = zc > 0 && finite_d(px) && finite_d(py) && finite_d(sx) && finite_d(sy);
      if (valid) {
        sx = fmax(sx, (double)a.sigma_floor);
        sy = fmax(sy, (double)a.sigma_floor);
        const double u = (a.K[0] * xc) / zc + a.K[2], v = (a.K[4] * yc) / zc + a.K[5];
        zx = (px - u) / sx;
        zy = (py - v) / sy;
        if (!finite_d(zx) || !finite_d(zy)) { valid = false; zx = zy = 0; }
      }
    }
    a.z[((size_t)b * Lm + lane) * 2] = zx;
    a.z[((size_t)b * Lm + lane) * 2 + 1] = zy;
    a.kp_flags[(size_t)b * Lm + lane] = (uint8_t)((valid ? 1 : 0) | (inlier ? 2 : 0));
  }
  if (lane != 0) return;

  double d[6] = {0, 0, 0, 0, 0, 0}, ne[3] = {0, 0, 0};
  int cs = 0;
  if (!have_pose) {
    cs = 2;
  } else {
    // q_pr = exp(rvec / 2); q_rel = q_pr (x) conj(q_gt) is the rotation R_pr R_gt^T
    double r[3], qp[4] = {1, 0, 0, 0};
    for (int i = 0; i < 3; ++i) r[i] = a.rvec[3 * b + i];
    const double th = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (!(th < DBL_EPSILON)) {
      double s, c;
      det_sincos(0.5 * th, &s, &c);
      const double k = s / th;
      qp[0] = c; qp[1] = r[0] * k; qp[2] = r[1] * k; qp[3] = r[2] * k;
    }
    double rw = qp[0] * w + (qp[1] * x + qp[2] * y + qp[3] * z);
    double rv[3] = {(w * qp[1] - qp[0] * x) - (qp[2] * z - qp[3] * y),
                    (w * qp[2] - qp[0] * y) - (qp[3] * x - qp[1] * z),
                    (w * qp[3] - qp[0] * z) - (qp[1] * y - qp[2] * x)};
    if (rw < 0) { rw = -rw; rv[0] = -rv[0]; rv[1] = -rv[1]; rv[2] = -rv[2]; }
    const double vn = sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
    const double k = vn > 0 ? 2.0 * atan2(vn, rw) / vn : 0.0;
    bool fin = true;
    for (int i = 0; i < 3; ++i) {
      d[i] = rv[i] * k;
      d[3 + i] = a.tvec[3 * b + i] - tg[i];
      fin = fin && finite_d(d[i]) && finite_d(d[3 + i]);
    }
    if (!fin)
      for (int i = 0; i < 6; ++i) d[i] = 0;
    if (a.cov_status[b] != 0) {
      cs = 3;
    } else if (!fin) {
      cs = 4;
    } else {
      double S[36];
      const double g2 = a.sigma_gain * a.sigma_gain;
      for (int i = 0; i < 36; ++i) S[i] = a.cov[(size_t)b * 36 + i] * g2;
      bool ok = nees6(S, d, &ne[0]) && nees3(S, 0, d, &ne[1]) && nees3(S, 3, d + 3, &ne[2]);
      ok = ok && finite_d(ne[0]) && finite_d(ne[1]) && finite_d(ne[2]);
      if (!ok) { cs = 4; ne[0] = ne[1] = ne[2] = 0; }
    }
  }
  for (int i = 0; i < 6; ++i) a.delta[6 * b + i] = d[i];
  for (int i = 0; i < 3; ++i) a.nees[3 * b + i] = ne[i];
  a.calib_status[b] = cs;
}

}  // namespace

int spe_launch_calib_records(const CalibArgs& a, hipStream_t s) {
  if (a.B <= 0) return 0;
  if (a.Q > WAVE || a.C < 2 || a.C - 1 > MAXN || !(a.sigma_floor > 0) || !(a.sigma_gain > 0)) return -7;
  hipLaunchKernelGGL(calib_records_kernel, dim3((a.B + CAL_WAVES - 1) / CAL_WAVES), dim3(WAVE * CAL_WAVES), 0, s, a);
  return (int)hipGetLastError();
}
