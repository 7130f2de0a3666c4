// Landmark reconstruction (definition: include/spe.h spe_landmarks_solve): the body-frame 3-D landmarks
// from 2-D keypoint observations in views of known pose, by a weighted linear triangulation and a fixed
// number of Huber-weighted Levenberg-Marquardt steps per landmark, with the covariance and the outlier
// flags.  The inverse of what the solvers do with the table, and what makes one (spe/landmarks.py).
//
// Two kernels alternate.  lm_accumulate_kernel: one lane per view, a loop over the landmarks; per landmark
// the LM_TERMS sums of the view at the current point are reduced across the wave by an xor butterfly
// (32, 16, .. 1: both partners add the same two numbers, so every lane holds the same bits) and lane 0
// stores the wave's partial.  lm_finalize_kernel: one wave per landmark; lane i adds the partials of waves
// i, i + 64, .. in that order, the same butterfly joins the lanes, and lane 0 decides, solves and updates
// the landmark's state.  No atomics, no LDS, no barrier: the summation order is a function of N alone and
// two runs give the same bits.  lm_flags_kernel marks the observations at the final point.
// lm_observations_kernel (spe_landmark_observations) is the solver's selection -- argmax_class /
// takes_over of pnp_math.h, as in calib.hip -- writing the observation layout.
// Compiled with -ffp-contract=off like calib.hip: every fp64 step rounds on its own, as the numpy
// restatement's does.
#include "spe_common.h"
#include "pnp_math.h"
#include "spe_pnp.h"

namespace {

constexpr int WAVE = 64;
constexpr int ACC_WAVES = 4;
constexpr int MAX_L = 16;
// the sums of one landmark: H or A (6, upper triangle by rows), g or b (3), cost, count, sum of px^2
constexpr int LM_TERMS = 12;
enum { T_COST = 9, T_COUNT = 10, T_PX2 = 11 };
enum { LM_LINEAR = 0, LM_EVAL = 1, LM_INIT = 2 };

// one landmark's state between the launches (in the caller's scratch)
struct LmState {
  double x[3];      // the accepted point
  double xt[3];     // the point the next accumulate evaluates
  double H[6], g[3], cost, px2;   // at x
  double lambda;
  int32_t n;        // views used at x
  int32_t status;
  int32_t have;     // x holds an evaluated point
  int32_t pad;
};

SPE_DEV bool finite_d(double x) { return fabs(x) < (double)INFINITY; }

SPE_DEV double wave_sum(double v) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

struct View {
  bool ok;
  double R[9], t[3];
};

SPE_DEV View load_view(const LandmarkArgs& a, int n, bool active) {
  View v;
  v.ok = false;
  for (int i = 0; i < 9; ++i) v.R[i] = 0;
  for (int i = 0; i < 3; ++i) v.t[i] = 0;
  if (!active) return v;
  double q[4], n2 = 0;
  for (int i = 0; i < 4; ++i) { q[i] = a.q_gt[(size_t)4 * n + i]; n2 += q[i] * q[i]; }
  for (int i = 0; i < 3; ++i) v.t[i] = a.t_gt[(size_t)3 * n + i];
  const double qn = sqrt(n2);
  v.ok = qn > 0 && finite_d(qn) && finite_d(v.t[0]) && finite_d(v.t[1]) && finite_d(v.t[2]);
  if (!v.ok) return v;
  const double w = q[0] / qn, x = q[1] / qn, y = q[2] / qn, z = q[3] / qn;
  v.R[0] = 1 - 2 * (y * y + z * z); v.R[1] = 2 * (x * y - z * w); v.R[2] = 2 * (x * z + y * w);
  v.R[3] = 2 * (x * y + z * w); v.R[4] = 1 - 2 * (x * x + z * z); v.R[5] = 2 * (y * z - x * w);
  v.R[6] = 2 * (x * z - y * w); v.R[7] = 2 * (y * z + x * w); v.R[8] = 1 - 2 * (x * x + y * y);
  return v;
}

// the observation of landmark l in view n and its effective sigma; false where it is skipped
SPE_DEV bool load_obs(const LandmarkArgs& a, int n, int l, double* p, double* s) {
  const size_t o = (size_t)n * a.L + l;
  if (!a.obs_valid[o]) return false;
  p[0] = a.obs_px[2 * o];
  p[1] = a.obs_px[2 * o + 1];
  s[0] = s[1] = 1.0;
  if (a.obs_sigma) { s[0] = a.obs_sigma[2 * o]; s[1] = a.obs_sigma[2 * o + 1]; }
  s[0] *= a.sigma_gain;
  s[1] *= a.sigma_gain;
  if (!(finite_d(p[0]) && finite_d(p[1]) && finite_d(s[0]) && finite_d(s[1]))) return false;
  s[0] = fmax(s[0], a.sigma_floor);
  s[1] = fmax(s[1], a.sigma_floor);
  return true;
}

// stage 0: the two weighted rows of the view into T
SPE_DEV void linear_terms(const View& v, const double* K, const double* p, const double* s, double* T) {
  const double uv[2] = {(p[0] - K[2]) / K[0], (p[1] - K[5]) / K[4]};
  const double f[2] = {K[0], K[4]};
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const double q = f[r] / s[r], w = q * q;
    const double c[3] = {v.R[3 * r] - uv[r] * v.R[6], v.R[3 * r + 1] - uv[r] * v.R[7], v.R[3 * r + 2] - uv[r] * v.R[8]};
    const double b = -(v.t[r] - uv[r] * v.t[2]);
    const double wc[3] = {w * c[0], w * c[1], w * c[2]};
    T[0] += wc[0] * c[0]; T[1] += wc[0] * c[1]; T[2] += wc[0] * c[2];
    T[3] += wc[1] * c[1]; T[4] += wc[1] * c[2]; T[5] += wc[2] * c[2];
    T[6] += wc[0] * b; T[7] += wc[1] * b; T[8] += wc[2] * b;
  }
  T[T_COUNT] = 1.0;
}

// stage 1: the view's residual at X.  -> 0 not used (depth <= z_min or not finite), 1 used, 3 used and
// beyond the Huber threshold (the obs_flags bits); T (nullable) receives the terms
SPE_DEV int eval_terms(const View& v, const double* K, const double* p, const double* s, const double* X,
                       double huber, double z_min, double* T) {
  const double xc = (v.R[0] * X[0] + v.R[1] * X[1] + v.R[2] * X[2]) + v.t[0];
  const double yc = (v.R[3] * X[0] + v.R[4] * X[1] + v.R[5] * X[2]) + v.t[1];
  const double zc = (v.R[6] * X[0] + v.R[7] * X[1] + v.R[8] * X[2]) + v.t[2];
  if (!(zc > z_min)) return 0;
  const double xz = xc / zc, yz = yc / zc;
  const double ex = p[0] - (K[0] * xz + K[2]), ey = p[1] - (K[4] * yz + K[5]);
  const double rx = ex / s[0], ry = ey / s[1];
  const double s2 = rx * rx + ry * ry;
  const double nr = sqrt(s2);
  if (!finite_d(nr)) return 0;
  double w = 1.0, rho = s2;
  int flag = 1;
  if (huber > 0 && nr > huber) {
    w = huber / nr;
    rho = 2.0 * huber * nr - huber * huber;
    flag = 3;
  }
  if (T) {
    const double ax = (K[0] / zc) / s[0], ay = (K[4] / zc) / s[1];
    const double jx[3] = {ax * (v.R[0] - xz * v.R[6]), ax * (v.R[1] - xz * v.R[7]), ax * (v.R[2] - xz * v.R[8])};
    const double jy[3] = {ay * (v.R[3] - yz * v.R[6]), ay * (v.R[4] - yz * v.R[7]), ay * (v.R[5] - yz * v.R[8])};
    T[0] = w * (jx[0] * jx[0] + jy[0] * jy[0]); T[1] = w * (jx[0] * jx[1] + jy[0] * jy[1]);
    T[2] = w * (jx[0] * jx[2] + jy[0] * jy[2]); T[3] = w * (jx[1] * jx[1] + jy[1] * jy[1]);
    T[4] = w * (jx[1] * jx[2] + jy[1] * jy[2]); T[5] = w * (jx[2] * jx[2] + jy[2] * jy[2]);
    T[6] = w * (jx[0] * rx + jy[0] * ry); T[7] = w * (jx[1] * rx + jy[1] * ry); T[8] = w * (jx[2] * rx + jy[2] * ry);
    T[T_COST] = rho;
    T[T_COUNT] = 1.0;
    T[T_PX2] = ex * ex + ey * ey;
  }
  return flag;
}

SPE_DEV LmState* states_of(void* scratch) { return (LmState*)scratch; }
SPE_DEV double* partials_of(void* scratch) { return (double*)((char*)scratch + MAX_L * sizeof(LmState)); }

__global__ __launch_bounds__(WAVE * ACC_WAVES) void lm_accumulate_kernel(LandmarkArgs a, int mode) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = blockIdx.x * ACC_WAVES + (int)(threadIdx.x / WAVE);
  const int waves = (a.N + WAVE - 1) / WAVE;
  if (wave >= waves) return;                          // wave-uniform
  const int n = wave * WAVE + lane;
  const bool active = n < a.N;
  const View v = load_view(a, n, active);
  const LmState* st = states_of(a.scratch);
  double* part = partials_of(a.scratch) + (size_t)wave * a.L * LM_TERMS;
  for (int l = 0; l < a.L; ++l) {
    double T[LM_TERMS];
#pragma unroll
    for (int k = 0; k < LM_TERMS; ++k) T[k] = 0;
    // a landmark with a status takes no further part (uniform; stage 0 writes the first status)
    const bool live = mode == LM_LINEAR || st[l].status == 0;
    double p[2], s[2];
    if (live && v.ok && load_obs(a, n, l, p, s)) {
      if (mode == LM_LINEAR) {
        linear_terms(v, a.K, p, s, T);
      } else {
        const double X[3] = {st[l].xt[0], st[l].xt[1], st[l].xt[2]};
        double E[LM_TERMS];
        if (eval_terms(v, a.K, p, s, X, a.huber, a.z_min, E)) {
#pragma unroll
          for (int k = 0; k < LM_TERMS; ++k) T[k] = E[k];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < LM_TERMS; ++k) T[k] = wave_sum(T[k]);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < LM_TERMS; ++k) part[l * LM_TERMS + k] = T[k];
    }
  }
}

// Cholesky factor of the Jacobi-scaled (H + lam diag H): A = D^-1/2 H D^-1/2 + lam I; sc = 1 / sqrt(diag H).
// false where a diagonal is not positive and finite or a pivot is <= 64 eps
SPE_DEV bool scaled_factor(const double* H6, double lam, double* sc, double (*Lc)[3]) {
  const double d[3] = {H6[0], H6[3], H6[5]};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (!(d[i] > 0) || !finite_d(d[i])) return false;
    sc[i] = 1.0 / sqrt(d[i]);
  }
  const double S[9] = {H6[0], H6[1], H6[2], H6[1], H6[3], H6[4], H6[2], H6[4], H6[5]};
  double A[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) A[i * 3 + j] = (S[i * 3 + j] * sc[i]) * sc[j] + (i == j ? lam : 0.0);
  return chol3_factor(A, 64.0 * DBL_EPSILON, Lc);
}

// x = (H + lam diag H)^-1 b through the factor
SPE_DEV void scaled_solve(const double (*Lc)[3], const double* sc, const double* b, double* x) {
  const double bs[3] = {b[0] * sc[0], b[1] * sc[1], b[2] * sc[2]};
  double y[3];
  chol3_backsolve(Lc, bs, y);
#pragma unroll
  for (int i = 0; i < 3; ++i) x[i] = y[i] * sc[i];
}

// -> the landmark's final status
SPE_DEV int write_outputs(const LandmarkArgs& a, int l, const LmState& s) {
  double C[9], x[3] = {0, 0, 0}, chi2 = 0, rms = 0;
  int n = 0, status = s.status;
#pragma unroll
  for (int i = 0; i < 9; ++i) C[i] = 0;
  if (status == 0) {
    double sc[3], Lc[3][3];
    if (!scaled_factor(s.H, 0.0, sc, Lc)) {
      status = 2;
    } else {
      bool fin = true;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double e[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
        double col[3];
        scaled_solve(Lc, sc, e, col);
#pragma unroll
        for (int i = 0; i <= j; ++i) { C[i * 3 + j] = col[i]; C[j * 3 + i] = col[i]; fin = fin && finite_d(col[i]); }
      }
      rms = sqrt(s.px2 / (double)s.n);
      fin = fin && finite_d(s.x[0]) && finite_d(s.x[1]) && finite_d(s.x[2]) && finite_d(s.cost) && finite_d(rms);
      if (!fin) status = 3;
    }
  }
  if (status == 0) {
    x[0] = s.x[0]; x[1] = s.x[1]; x[2] = s.x[2];
    chi2 = s.cost;
    n = s.n;
  } else {
    rms = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) C[i] = 0;
  }
  for (int i = 0; i < 3; ++i) a.world[3 * l + i] = x[i];
  for (int i = 0; i < 9; ++i) a.cov[9 * l + i] = C[i];
  a.chi2[l] = chi2;
  a.n_used[l] = n;
  a.rms_px[l] = rms;
  a.lm_status[l] = status;
  return status;
}

__global__ __launch_bounds__(WAVE) void lm_finalize_kernel(LandmarkArgs a, int mode, int last) {
  const int lane = threadIdx.x;
  const int l = blockIdx.x;
  if (l >= a.L) return;
  double T[LM_TERMS];
#pragma unroll
  for (int k = 0; k < LM_TERMS; ++k) T[k] = 0;
  if (mode != LM_INIT) {
    const int waves = (a.N + WAVE - 1) / WAVE;
    const double* part = partials_of(a.scratch);
    for (int w = lane; w < waves; w += WAVE) {
      const double* p = part + ((size_t)w * a.L + l) * LM_TERMS;
#pragma unroll
      for (int k = 0; k < LM_TERMS; ++k) T[k] += p[k];
    }
#pragma unroll
    for (int k = 0; k < LM_TERMS; ++k) T[k] = wave_sum(T[k]);
  }
  if (lane != 0) return;
  LmState* sp = states_of(a.scratch) + l;
  LmState s;
  if (mode == LM_EVAL) {
    s = *sp;
  } else {
    for (int i = 0; i < 3; ++i) s.x[i] = s.xt[i] = s.g[i] = 0;
    for (int i = 0; i < 6; ++i) s.H[i] = 0;
    s.cost = s.px2 = 0;
    s.lambda = 1e-3;
    s.n = s.status = s.have = s.pad = 0;
  }
  if (mode == LM_INIT) {
    for (int i = 0; i < 3; ++i) s.xt[i] = a.world_init[3 * l + i];
    if (!(finite_d(s.xt[0]) && finite_d(s.xt[1]) && finite_d(s.xt[2]))) s.status = 3;
  } else if (mode == LM_LINEAR) {
    double sc[3], Lc[3][3];
    if ((int)T[T_COUNT] < 2) {
      s.status = 1;
    } else if (!scaled_factor(T, 0.0, sc, Lc)) {
      s.status = 2;
    } else {
      scaled_solve(Lc, sc, T + 6, s.xt);
      if (!(finite_d(s.xt[0]) && finite_d(s.xt[1]) && finite_d(s.xt[2]))) s.status = 3;
    }
  } else if (s.status == 0) {
    const int n = (int)T[T_COUNT];
    bool accept;
    if (!s.have) {
      accept = n >= 2;
      if (!accept) s.status = 1;
    } else {
      accept = T[T_COST] < s.cost && n >= s.n;
      s.lambda = accept ? s.lambda / 10.0 : s.lambda * 10.0;
    }
    if (accept) {
      for (int i = 0; i < 3; ++i) { s.x[i] = s.xt[i]; s.g[i] = T[6 + i]; }
      for (int i = 0; i < 6; ++i) s.H[i] = T[i];
      s.cost = T[T_COST];
      s.px2 = T[T_PX2];
      s.n = n;
      s.have = 1;
    }
    if (s.status == 0 && !last) {
      double sc[3], Lc[3][3], d[3];
      if (!scaled_factor(s.H, s.lambda, sc, Lc)) {
        s.status = 2;
      } else {
        scaled_solve(Lc, sc, s.g, d);
        for (int i = 0; i < 3; ++i) s.xt[i] = s.x[i] + d[i];
        if (!(finite_d(s.xt[0]) && finite_d(s.xt[1]) && finite_d(s.xt[2]))) s.status = 3;
      }
    }
  }
  if (last) s.status = write_outputs(a, l, s);
  *sp = s;
}

// obs_flags at the accepted points, one lane per view
__global__ __launch_bounds__(WAVE * ACC_WAVES) void lm_flags_kernel(LandmarkArgs a) {
  const int n = blockIdx.x * (WAVE * ACC_WAVES) + threadIdx.x;
  if (n >= a.N) return;
  const View v = load_view(a, n, true);
  const LmState* st = states_of(a.scratch);
  for (int l = 0; l < a.L; ++l) {
    int flag = 0;
    double p[2], s[2];
    if (st[l].status == 0 && v.ok && load_obs(a, n, l, p, s)) {
      const double X[3] = {st[l].x[0], st[l].x[1], st[l].x[2]};
      flag = eval_terms(v, a.K, p, s, X, a.huber, a.z_min, nullptr);
    }
    a.obs_flags[(size_t)n * a.L + l] = (uint8_t)flag;
  }
}

__global__ __launch_bounds__(WAVE * ACC_WAVES) void lm_observations_kernel(LandmarkObsArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int b = blockIdx.x * ACC_WAVES + (int)(threadIdx.x / WAVE);
  if (b >= a.B) return;                               // wave-uniform
  const int Q = a.Q, C = a.C, Lm = C - 1;
  // selection, as in calib_records_kernel
  int lab_q = C - 1;
  float sc_q = 0.f;
  if (lane < Q) lab_q = argmax_class(a.probs + ((size_t)b * Q + lane) * C, C, &sc_q);
  const int mylab = lane < Lm ? lane : -1;
  int best_q = -1;
  float best_s = 0.f;
  for (int q = 0; q < Q; ++q) {
    const int l = __shfl(lab_q, q);
    const float s = __shfl(sc_q, q);
    if (l == mylab && takes_over(best_q, best_s, s)) { best_q = q; best_s = s; }
  }
  if (lane >= Lm) return;
  const size_t o = (a.row_offset + (size_t)b) * Lm + lane;
  double px = 0, py = 0, sx = 1, sy = 1;
  if (best_q >= 0) {
    const size_t i = ((size_t)b * Q + best_q) * 2;
    px = (double)a.points[i];
    py = (double)a.points[i + 1];
    if (a.sigmas) {
      sx = (double)a.sigmas[i];
      sy = (double)a.sigmas[i + 1];
      if (a.sigma_scale) { sx *= (double)a.sigma_scale[2 * b]; sy *= (double)a.sigma_scale[2 * b + 1]; }
    }
  }
  a.obs_px[2 * o] = px;
  a.obs_px[2 * o + 1] = py;
  if (a.obs_sigma) { a.obs_sigma[2 * o] = sx; a.obs_sigma[2 * o + 1] = sy; }
  a.obs_valid[o] = best_q >= 0 ? 1 : 0;
}

}  // namespace

size_t spe_landmarks_scratch_size(int N, int L) {
  if (N < 1 || L < 1 || L > MAX_L) return 0;
  const size_t waves = ((size_t)N + WAVE - 1) / WAVE;
  return MAX_L * sizeof(LmState) + waves * (size_t)L * LM_TERMS * sizeof(double);
}

int spe_launch_landmark_observations(const LandmarkObsArgs& a, hipStream_t s) {
  if (a.B <= 0) return 0;
  if (a.Q < 1 || a.Q > WAVE || a.C < 2 || a.C - 1 > MAX_L) return -7;
  hipLaunchKernelGGL(lm_observations_kernel, dim3((a.B + ACC_WAVES - 1) / ACC_WAVES), dim3(WAVE * ACC_WAVES), 0, s, a);
  return (int)hipGetLastError();
}

int spe_launch_landmarks_solve(const LandmarkArgs& a, hipStream_t s) {
  if (a.N < 1 || a.L < 1 || a.L > MAX_L || a.iterations < 0 || a.iterations > 64 || !a.scratch) return -7;
  const int waves = (a.N + WAVE - 1) / WAVE;
  const dim3 acc_grid((waves + ACC_WAVES - 1) / ACC_WAVES), acc_block(WAVE * ACC_WAVES);
  // the start point: the caller's, or stage 0
  if (a.world_init) {
    hipLaunchKernelGGL(lm_finalize_kernel, dim3(a.L), dim3(WAVE), 0, s, a, (int)LM_INIT, 0);
  } else {
    hipLaunchKernelGGL(lm_accumulate_kernel, acc_grid, acc_block, 0, s, a, (int)LM_LINEAR);
    hipLaunchKernelGGL(lm_finalize_kernel, dim3(a.L), dim3(WAVE), 0, s, a, (int)LM_LINEAR, 0);
  }
  // its evaluation, then one pair per step: pair k evaluates step k's candidate and makes step k + 1's
  for (int k = 0; k <= a.iterations; ++k) {
    hipLaunchKernelGGL(lm_accumulate_kernel, acc_grid, acc_block, 0, s, a, (int)LM_EVAL);
    hipLaunchKernelGGL(lm_finalize_kernel, dim3(a.L), dim3(WAVE), 0, s, a, (int)LM_EVAL, k == a.iterations ? 1 : 0);
  }
  hipLaunchKernelGGL(lm_flags_kernel, dim3((a.N + WAVE * ACC_WAVES - 1) / (WAVE * ACC_WAVES)), acc_block, 0, s, a);
  return (int)hipGetLastError();
}
