// Multi-checkpoint ensemble front end on the device: Multi_Mean_PoseSolver's
// keypoint fusion (REV/utils/speed_eval.py:42-100) for a whole batch, feeding the same batched
// P3P-RANSAC + LM solve as the single-model path (spe_pnp_batch).
//
// Per image: for every model, label = argmax of its PostProcess probabilities (background
// dropped); points are pooled per label in model-then-query order, labels in first-seen order;
// each label's fused point is the float32 mean of its points, or -- with 3 or more points --
// the float32 mean of those closer than 3 std (population, fp64) of the fp64 distances to that
// mean (mean_and_filter, :54-71).  numpy's reduction orders are followed exactly (row-by-row
// float32 axis-0 sums, pairwise fp64 sums for the 1-D std), so results equal the restatement in
// oracle/ensemble_ref.py bit for bit (this file is built with -ffp-contract=off).  Output rows
// are laid out for spe_pnp_batch's selection: row i = i-th first-seen label with a one-hot
// probability row, the remaining rows background.  One thread per image (M * Q <= a few hundred
// points): the fusion is a tiny prologue to the fp64 solver.
#include <limits.h>

#include "spe_common.h"
#include "spe_kernels.h"

namespace {

constexpr int KMAX = 16;     // labels (num_classes - 1)

// numpy's pairwise summation (pairwise_sum_DOUBLE, block size 128) of the n fp64 values f(off) ..
// f(off + n - 1).  One unsplit block, n <= 128: sequential below 8 values, 8 accumulators above.
template <typename F>
SPE_DEV double pairwise_block(int off, int n, F f) {
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += f(off + i);
    return r;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = f(off + j);
  int i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] += f(off + i + j);
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += f(off + i);
  return res;
}

// Above 128 values numpy splits: n2 = n / 2 rounded down to a multiple of 8, sum(a, n2) +
// sum(a + n2, n - n2).  This level takes n <= 136 (both halves are single blocks) ...
template <typename F>
SPE_DEV double pairwise_split(int off, int n, F f) {
  if (n <= 128) return pairwise_block(off, n, f);
  int n2 = n / 2;
  n2 -= n2 % 8;
  return pairwise_block(off, n2, f) + pairwise_block(off + n2, n - n2, f);
}

// ... and this one n <= 256, the contract's M * Q: the first half is at most 128 values, the second at
// most 136 (n = 250 .. 255 leave 130 .. 135 there, which split once more).  Written out instead of
// recursing so that the kernel needs no call stack.
template <typename F>
SPE_DEV double pairwise_sum(int n, F f) {
  if (n <= 128) return pairwise_block(0, n, f);
  int n2 = n / 2;
  n2 -= n2 % 8;
  return pairwise_block(0, n2, f) + pairwise_split(n2, n - n2, f);
}

__global__ __launch_bounds__(64) void ensemble_fuse_kernel(EnsembleArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  const int M = a.M, Q = a.Q, C = a.C, K = C - 1;
  // first-seen label order and each query's label
  int order[KMAX], nl = 0;
  bool seen[KMAX];
  for (int k = 0; k < K; ++k) seen[k] = false;
  auto label_of = [&](int m, int q) {
    const float* p = a.probs + (((size_t)m * a.B + b) * Q + q) * C;
    int am = 0;
    float mx = p[0];
    for (int c = 1; c < C; ++c)
      if (p[c] > mx) { mx = p[c]; am = c; }
    return am;
  };
  for (int m = 0; m < M; ++m)
    for (int q = 0; q < Q; ++q) {
      const int l = label_of(m, q);
      if (l != K && !seen[l]) { seen[l] = true; order[nl++] = l; }
    }
  float* outp = a.fused_points + (size_t)b * K * 2;
  float* outr = a.fused_probs + (size_t)b * K * C;
  for (int i = 0; i < K; ++i)
    for (int c = 0; c < C; ++c) outr[i * C + c] = c == K ? 1.f : 0.f;
  for (int i = 0; i < nl; ++i) {
    const int l = order[i];
    // pass 1: float32 row-by-row mean of the label's points
    float sx = 0.f, sy = 0.f;
    int n = 0;
    for (int m = 0; m < M; ++m)
      for (int q = 0; q < Q; ++q)
        if (label_of(m, q) == l) {
          const float* pt = a.points + (((size_t)m * a.B + b) * Q + q) * 2;
          sx = sx + pt[0];
          sy = sy + pt[1];
          ++n;
        }
    float fx = sx / (float)n, fy = sy / (float)n;
    if (n >= 3) {
      // fp64 distances to the mean, in pooling order (<= M * Q of them)
      double d[256];
      int nd = 0;
      for (int m = 0; m < M; ++m)
        for (int q = 0; q < Q; ++q)
          if (label_of(m, q) == l && nd < 256) {
            const float* pt = a.points + (((size_t)m * a.B + b) * Q + q) * 2;
            const double dx = (double)pt[0] - (double)fx, dy = (double)pt[1] - (double)fy;
            d[nd++] = sqrt(dx * dx + dy * dy);
          }
      const double mu = pairwise_sum(nd, [&](int j) { return d[j]; }) / nd;
      const double sd = sqrt(pairwise_sum(nd, [&](int j) { return (d[j] - mu) * (d[j] - mu); }) / nd);
      float kx = 0.f, ky = 0.f;
      int nk = 0, j = 0;
      for (int m = 0; m < M; ++m)
        for (int q = 0; q < Q; ++q)
          if (label_of(m, q) == l) {
            if (d[j] < sd * 3) {
              const float* pt = a.points + (((size_t)m * a.B + b) * Q + q) * 2;
              kx = kx + pt[0];
              ky = ky + pt[1];
              ++nk;
            }
            ++j;
          }
      // np.mean of an empty selection (every distance >= 3 std, e.g. coinciding points with
      // std 0) is NaN, like the reference: 0 / 0 here
      fx = kx / (float)nk;
      fy = ky / (float)nk;
    }
    outp[2 * i] = fx;
    outp[2 * i + 1] = fy;
    outr[i * C + K] = 0.f;
    outr[i * C + l] = 1.f;
  }
  for (int i = nl; i < K; ++i) { outp[2 * i] = 0.f; outp[2 * i + 1] = 0.f; }
}

// ---------------------------------------------------------------- sigma-weighted fusion
// spe_ensemble_fuse_sigma (definition: include/spe.h).  One wavefront per image, three phases:
//   1. lanes stride over the M * Q probability rows: label and score of each, once, into LDS;
//   2. lanes stride over the M * K (model, label) pairs: the label's best query of that model, its
//      point and effective sigma (fp64) into LDS;
//   3. lane l owns label l: the gated weighted mean in the definition's fp64 order, the label's rank
//      among the emitted ones from a compare across the K lanes, one output row per lane.
constexpr int MMAX = 16;     // models
constexpr int RMAX = 256;    // M * Q probability rows

struct FuseSigmaShared {
  double x[MMAX][KMAX], y[MMAX][KMAX], sx[MMAX][KMAX], sy[MMAX][KMAX];
  float score[RMAX];               // phase 1: per row
  float msc[MMAX][KMAX];           // phase 2: the measurement's score
  int pos[KMAX];                   // first-seen position of an emitted label, INT_MAX otherwise
  short firstq[MMAX][KMAX];        // the model's first query with the label
  unsigned char lab[RMAX];
  unsigned char state[MMAX][KMAX]; // 0 the model lacks the label, 1 measurement not usable, 2 usable
};

__global__ __launch_bounds__(64) void ensemble_fuse_sigma_kernel(EnsembleSigmaArgs a) {
  __shared__ FuseSigmaShared sh;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int M = a.M, B = a.B, Q = a.Q, C = a.C, K = C - 1;
  for (int r = lane; r < M * Q; r += 64) {
    const int m = r / Q, q = r - m * Q;
    const float* p = a.probs + (((size_t)m * B + b) * Q + q) * C;
    int am = 0;
    float mx = p[0];
    for (int c = 1; c < C; ++c)
      if (p[c] > mx) { mx = p[c]; am = c; }
    sh.lab[r] = (unsigned char)am;
    sh.score[r] = mx;
  }
  __syncthreads();
  double scx = 1.0, scy = 1.0;
  if (a.sigma_scale) { scx = (double)a.sigma_scale[2 * (size_t)b]; scy = (double)a.sigma_scale[2 * (size_t)b + 1]; }
  const bool scale_ok = isfinite(scx) && isfinite(scy) && scx > 0.0 && scy > 0.0;
  const double floor_d = (double)a.sigma_floor;
  for (int pr = lane; pr < M * K; pr += 64) {
    const int m = pr / K, l = pr - m * K;
    int first = -1, best = -1;
    float bs = 0.f;
    for (int q = 0; q < Q; ++q)
      if (sh.lab[m * Q + q] == l) {
        const float sc = sh.score[m * Q + q];
        if (first < 0) first = q;
        if (best < 0 || sc > bs) { best = q; bs = sc; }
      }
    unsigned char st = 0;
    if (best >= 0) {
      st = 1;
      const size_t r = ((size_t)m * B + b) * Q + best;
      const float px = a.points[2 * r], py = a.points[2 * r + 1];
      const double ux = (double)a.sigmas[2 * r] * scx, uy = (double)a.sigmas[2 * r + 1] * scy;
      if (scale_ok && isfinite(px) && isfinite(py) && isfinite(ux) && isfinite(uy) && isfinite(bs)) {
        st = 2;
        sh.x[m][l] = (double)px;
        sh.y[m][l] = (double)py;
        sh.sx[m][l] = ux > floor_d ? ux : floor_d;
        sh.sy[m][l] = uy > floor_d ? uy : floor_d;
        sh.msc[m][l] = bs;
      }
    }
    sh.state[m][l] = st;
    sh.firstq[m][l] = (short)first;
  }
  __syncthreads();
  const int l = lane;
  int pos = INT_MAX, npool = 0, n = 0;
  unsigned kept = 0;
  double mux = 0.0, muy = 0.0, swx = 0.0, swy = 0.0;
  if (l < K) {
    for (int m = 0; m < M; ++m) {
      const int st = sh.state[m][l];
      if (st && pos == INT_MAX) pos = m * Q + sh.firstq[m][l];
      npool += st != 0;
      if (st == 2) kept |= 1u << m;
    }
    if (!kept) pos = INT_MAX;
    // every pass drops one measurement or ends: at most M - 2 drops
    for (int pass = 0; pass < M && kept; ++pass) {
      double ax = 0.0, ay = 0.0;
      swx = 0.0;
      swy = 0.0;
      for (int m = 0; m < M; ++m)
        if (kept >> m & 1) {
          const double wx = 1.0 / (sh.sx[m][l] * sh.sx[m][l]), wy = 1.0 / (sh.sy[m][l] * sh.sy[m][l]);
          swx = swx + wx;
          swy = swy + wy;
          ax = ax + wx * sh.x[m][l];
          ay = ay + wy * sh.y[m][l];
        }
      mux = ax / swx;
      muy = ay / swy;
      n = __popc(kept);
      if (n < 3) break;
      double dmax = -1.0;
      int im = 0;
      for (int m = 0; m < M; ++m)
        if (kept >> m & 1) {
          const double dx = (sh.x[m][l] - mux) / sh.sx[m][l], dy = (sh.y[m][l] - muy) / sh.sy[m][l];
          const double d2 = dx * dx + dy * dy;
          if (d2 > dmax) { dmax = d2; im = m; }
        }
      if (!(sqrt(dmax) > (double)a.gate)) break;
      kept &= ~(1u << im);
    }
    sh.pos[l] = pos;
  }
  __syncthreads();
  if (l >= K) return;
  // row: an emitted label's rank in first-seen order; the others fill the rows behind, background
  const bool emitted = kept != 0;
  int before = 0, n_emitted = 0, unused_before = 0;
  for (int j = 0; j < K; ++j) {
    const int pj = sh.pos[j];
    n_emitted += pj != INT_MAX;
    before += pj < pos;
    unused_before += pj == INT_MAX && j < l;
  }
  const int row = emitted ? before : n_emitted + unused_before;
  float fx = 0.f, fy = 0.f, gx = 0.f, gy = 0.f, fsc = 0.f;
  if (emitted) {
    double cx = 0.0, cy = 0.0, ss = 0.0;
    for (int m = 0; m < M; ++m)
      if (kept >> m & 1) {
        const double wx = 1.0 / (sh.sx[m][l] * sh.sx[m][l]), wy = 1.0 / (sh.sy[m][l] * sh.sy[m][l]);
        const double ex = sh.x[m][l] - mux, ey = sh.y[m][l] - muy;
        cx = cx + wx * (ex * ex);
        cy = cy + wy * (ey * ey);
        ss = ss + (double)sh.msc[m][l];
      }
    double bx = 1.0, by = 1.0;
    if (n > 1) {
      bx = sqrt(cx / (double)(n - 1));
      by = sqrt(cy / (double)(n - 1));
      if (!(bx > 1.0)) bx = 1.0;
      if (!(by > 1.0)) by = 1.0;
    }
    fx = (float)mux;
    fy = (float)muy;
    gx = (float)(sqrt(1.0 / swx) * bx / scx);
    gy = (float)(sqrt(1.0 / swy) * by / scy);
    fsc = (float)(ss / (double)n);
  }
  const size_t o = (size_t)b * K + row;
  a.fused_points[2 * o] = fx;
  a.fused_points[2 * o + 1] = fy;
  a.fused_sigmas[2 * o] = gx;
  a.fused_sigmas[2 * o + 1] = gy;
  a.n_pooled[o] = emitted ? npool : 0;
  a.n_kept[o] = emitted ? n : 0;
  float* pr = a.fused_probs + o * C;
  for (int c = 0; c < C; ++c) pr[c] = emitted ? (c == l ? fsc : 0.f) : (c == K ? 1.f : 0.f);
}

}  // namespace

int spe_launch_ensemble_fuse_sigma(const EnsembleSigmaArgs& a, hipStream_t s) {
  if (a.B < 1 || a.M < 1 || a.M > MMAX || a.Q < 1 || a.C < 2 || a.C - 1 > KMAX || (size_t)a.M * a.Q > RMAX) return -5;
  hipLaunchKernelGGL(ensemble_fuse_sigma_kernel, dim3(a.B), dim3(64), 0, s, a);
  return (int)hipGetLastError();
}

int spe_launch_ensemble_fuse(const EnsembleArgs& a, hipStream_t s) {
  if (a.B <= 0) return 0;
  if (a.M < 1 || a.Q < 1 || a.C < 2 || a.C - 1 > KMAX || (size_t)a.M * a.Q > 256) return -5;
  hipLaunchKernelGGL(ensemble_fuse_kernel, dim3((a.B + 63) / 64), dim3(64), 0, s, a);
  return (int)hipGetLastError();
}
