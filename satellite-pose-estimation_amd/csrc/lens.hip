// Lens distortion in front of the solvers (include/spe.h: spe_undistort_points, spe_distort_points).
//
// The solver kernels work on a pinhole camera and are pinned bit for bit against OpenCV's control
// flow, so distortion is not threaded through them: undistort_kernel turns distorted pixel points into
// ideal pixel points K . undistort(K^-1 p) and carries the per-axis pixel sigma through the same map;
// every solver, the self-assessment, the covariance and the ensemble then run unchanged.
//
// Model: OpenCV's five coefficients (k1, k2, p1, p2, k3), fp64 throughout.  The undistortion is
// cv2.undistortPoints' fixed-point iteration run for exactly `iters` rounds, without its early exit on
// a tolerance.  PARITY UNPINNED: cv2 is absent here, the kernel is checked against a numpy restatement
// of include/spe.h's definition (tests/lens_ref.py).
//
// Sigma: with D the 2x2 Jacobian of the distort map in pixels at the undistorted point and A = D^-1,
// the ideal covariance is A Sigma A^T.  Its cross term is dropped: the solvers and the covariance take
// one sigma per axis, so only the diagonal is returned.
//
// One thread per point, one launch, no LDS, no scratch, no barrier.  A few hundred fp64 operations on
// B * Q points: the launch is the cost, so there is nothing to tune beyond the coalesced float2 moves.
// Compiled without FMA contraction (Makefile): each fp64 step rounds as the restatement's does.
#include <math.h>

#include "spe_common.h"
#include "spe_kernels.h"

namespace {

constexpr int LENS_BLOCK = 256;

struct Lens {
  double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

__device__ inline Lens load_lens(const double* K, const double* d) {
  return Lens{K[0], K[4], K[2], K[5], d[0], d[1], d[2], d[3], d[4]};
}

__device__ inline bool positive_finite(double v) { return v > 0.0 && v < (double)INFINITY; }

__device__ inline double radial(const Lens& L, double r2) { return 1.0 + ((L.k3 * r2 + L.k2) * r2 + L.k1) * r2; }

__global__ __launch_bounds__(LENS_BLOCK) void undistort_kernel(LensArgs a) {
  const size_t i = (size_t)blockIdx.x * LENS_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const float2 p = reinterpret_cast<const float2*>(a.points)[i];
  float2 s = make_float2(0.f, 0.f);
  if (a.sigmas) s = reinterpret_cast<const float2*>(a.sigmas)[i];
  float2 po = p, so = s;
  uint8_t st = 0;
  const Lens L = load_lens(a.K, a.dist);
  // zero distortion is a copy, not (u - cx) / fx * fx + cx
  if (L.k1 != 0.0 || L.k2 != 0.0 || L.p1 != 0.0 || L.p2 != 0.0 || L.k3 != 0.0) {
    const double x0 = ((double)p.x - L.cx) / L.fx, y0 = ((double)p.y - L.cy) / L.fy;
    double x = x0, y = y0;
    bool ok = true;
    for (int it = 0; it < a.iters; ++it) {
      const double r2 = x * x + y * y;
      const double icd = 1.0 / radial(L, r2);
      if (!positive_finite(icd)) { ok = false; break; }
      const double dx = 2.0 * L.p1 * x * y + L.p2 * (r2 + 2.0 * x * x);
      const double dy = L.p1 * (r2 + 2.0 * y * y) + 2.0 * L.p2 * x * y;
      x = (x0 - dx) * icd;
      y = (y0 - dy) * icd;
    }
    if (ok) {
      // D = d(ud, vd) / d(ui, vi) at (x, y), the fx / fy factors included
      const double r2 = x * x + y * y;
      const double rad = radial(L, r2);
      const double g = (3.0 * L.k3 * r2 + 2.0 * L.k2) * r2 + L.k1;
      const double c = 2.0 * x * y * g + 2.0 * L.p1 * x + 2.0 * L.p2 * y;
      const double d11 = rad + 2.0 * x * x * g + 2.0 * L.p1 * y + 6.0 * L.p2 * x;
      const double d22 = rad + 2.0 * y * y * g + 6.0 * L.p1 * y + 2.0 * L.p2 * x;
      const double d12 = c * (L.fx / L.fy), d21 = c * (L.fy / L.fx);
      const double det = d11 * d22 - d12 * d21;
      ok = positive_finite(fabs(det));
      if (ok) {
        po = make_float2((float)(L.fx * x + L.cx), (float)(L.fy * y + L.cy));
        if (a.sigmas) {
          double sx = 1.0, sy = 1.0;
          if (a.sigma_scale) {
            const size_t b = i / (size_t)a.Q;
            sx = (double)a.sigma_scale[2 * b];
            sy = (double)a.sigma_scale[2 * b + 1];
          }
          const double ux = (double)s.x * sx, uy = (double)s.y * sy;
          const double a11 = d22 / det, a12 = -d12 / det, a21 = -d21 / det, a22 = d11 / det;
          so = make_float2((float)(sqrt((a11 * a11) * (ux * ux) + (a12 * a12) * (uy * uy)) / sx),
                           (float)(sqrt((a21 * a21) * (ux * ux) + (a22 * a22) * (uy * uy)) / sy));
        }
      }
    }
    st = ok ? 0 : 1;
  }
  reinterpret_cast<float2*>(a.points_out)[i] = po;
  if (a.sigmas_out) reinterpret_cast<float2*>(a.sigmas_out)[i] = so;
  if (a.status) a.status[i] = st;
}

__global__ __launch_bounds__(LENS_BLOCK) void distort_kernel(LensArgs a) {
  const size_t i = (size_t)blockIdx.x * LENS_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const float2 p = reinterpret_cast<const float2*>(a.points)[i];
  const Lens L = load_lens(a.K, a.dist);
  const double x = ((double)p.x - L.cx) / L.fx, y = ((double)p.y - L.cy) / L.fy;
  const double r2 = x * x + y * y;
  const double rad = radial(L, r2);
  const double xd = x * rad + 2.0 * L.p1 * x * y + L.p2 * (r2 + 2.0 * x * x);
  const double yd = y * rad + L.p1 * (r2 + 2.0 * y * y) + 2.0 * L.p2 * x * y;
  reinterpret_cast<float2*>(a.points_out)[i] = make_float2((float)(L.fx * xd + L.cx), (float)(L.fy * yd + L.cy));
}

unsigned lens_grid(size_t n) { return (unsigned)((n + LENS_BLOCK - 1) / LENS_BLOCK); }

}  // namespace

int spe_launch_undistort_points(const LensArgs& a, hipStream_t s) {
  if (a.n < 1 || a.n > ((size_t)1 << 30) || a.Q < 1 || a.iters < 1) return -5;
  hipLaunchKernelGGL(undistort_kernel, dim3(lens_grid(a.n)), dim3(LENS_BLOCK), 0, s, a);
  return (int)hipGetLastError();
}

int spe_launch_distort_points(const LensArgs& a, hipStream_t s) {
  if (a.n < 1 || a.n > ((size_t)1 << 30)) return -5;
  hipLaunchKernelGGL(distort_kernel, dim3(lens_grid(a.n)), dim3(LENS_BLOCK), 0, s, a);
  return (int)hipGetLastError();
}
