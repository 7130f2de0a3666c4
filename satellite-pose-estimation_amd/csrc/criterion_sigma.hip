// Set criterion of the UNC RT-DETR sigma model on the device: HungarianMatcher +
// SetCriterion losses for the main output, every aux decoder layer and the encoder top-k entry
// (UNC/src/zoo/rtdetr/rtdetr_criterion.py:103-213, 280-337, matcher.py:53-117; the logging half
// of UNC/solver/speed_engine.py:145-173).
//
//   cost[q][t] = cost_bbox * (|px - tx| + |py - ty|) + cost_class * (-prob_q[label_t])
//                prob = sigmoid(logit) with sigmoid_cost (the speed configs' use_focal_loss),
//                else softmax(logits_q); fp32 in torch's order, assignment minimising the fp64
//                sum (scipy's linear_sum_assignment, criterion_lsap.h)
//   loss_ce            weighted cross entropy over all queries (unmatched -> class C-1, weight
//                      eos_coef), class_error = 100 - top-1 accuracy of the matched queries,
//   cardinality_error  mean |#queries not predicting class C-1 - #targets|,
//   loss_bbox          both reference forms over matched pairs and both axes / num_boxes:
//                      points  |p - t|;  points_uncert  |p - t| * exp(-s) + 0.5 * s with s the
//                      layer's log sigma, 0 for a layer without one (the encoder top-k entry),
//   points_different   sum (p - t).
//
// The scheme is criterion.hip's: one wave per (layer, image), lanes build the cost matrix and the
// per-query terms, lane 0 runs the assignment in LDS, and a second launch reduces the per-image
// partial sums per layer in image order (deterministic).  The per-element terms are fp32 like the
// reference's, their sums fp64.
#include "spe_common.h"
#include "spe_kernels.h"
#include "criterion_lsap.h"

namespace {

constexpr int QMAX = 64, TMAX = 32, CMAX = 64, NPART = 8;

__global__ __launch_bounds__(64) void criterion_sigma_match_kernel(CritSigmaArgs a) {
  const int lb = blockIdx.x, l = lb / a.B, b = lb - l * a.B, q = threadIdx.x;
  const int Q = a.Q, T = a.T, C = a.C;
  __shared__ double cost[QMAX * TMAX];
  __shared__ int tclass[QMAX], amax[QMAX], tlab[TMAX];
  __shared__ int col4row[QMAX], row4col[QMAX], path[QMAX], remaining[QMAX];
  __shared__ double u[QMAX], v[QMAX], spc[QMAX];
  __shared__ bool sr[QMAX], sc[QMAX];
  __shared__ int mq[TMAX];
  const size_t row0 = ((size_t)l * a.B + b) * Q;
  const float* lg = a.logits + row0 * C;
  const float* pt = a.points + row0 * 2;
  const float* ls = a.log_sigmas && a.layer_has_sigma[l] ? a.log_sigmas + row0 * 2 : nullptr;
  const float* tp = a.tgt_points + (size_t)b * T * 2;
  if (q < T) {
    // a label outside [0, C) counts as no-object: it never indexes past a logits row
    const int lab = a.tgt_labels[(size_t)b * T + q];
    tlab[q] = lab >= 0 && lab < C ? lab : C - 1;
  }
  __syncthreads();
  float lse = 0.f, mx = 0.f;
  if (q < Q) {
    // log-sum-exp for the cross entropy and the softmax cost (fp32: max, exp(x - max), sum)
    mx = lg[q * C];
    int am = 0;
    for (int k = 1; k < C; ++k)
      if (lg[q * C + k] > mx) { mx = lg[q * C + k]; am = k; }
    float s = 0.f;
    for (int k = 0; k < C; ++k) s += expf(lg[q * C + k] - mx);
    lse = logf(s);
    amax[q] = am;
    tclass[q] = C - 1;                       // no-object unless matched
    const float px = pt[2 * q], py = pt[2 * q + 1];
    // cost in the matcher's orientation [Q][T], or transposed [T][Q] when Q > T (scipy)
    for (int t = 0; t < T; ++t) {
      const float x = lg[q * C + tlab[t]];
      const float pr = a.sigmoid_cost ? 1.f / (1.f + expf(-x)) : expf(x - mx) / s;
      const float cp = fabsf(px - tp[2 * t]) + fabsf(py - tp[2 * t + 1]);
      const float cc = -pr;
      const float cst = a.cost_bbox * cp + a.cost_class * cc;
      if (Q > T) cost[t * Q + q] = (double)cst;
      else cost[q * T + t] = (double)cst;
    }
  }
  __syncthreads();
  if (q == 0) {
    const bool tr = Q > T;
    lsap_lane(cost, tr ? T : Q, tr ? Q : T, col4row, row4col, u, v, spc, path, sr, sc, remaining);
    for (int t = 0; t < T; ++t) mq[t] = -1;
    if (tr) {
      for (int t = 0; t < T; ++t) mq[t] = col4row[t];
    } else {
      for (int qq = 0; qq < Q; ++qq)
        if (col4row[qq] >= 0) mq[col4row[qq]] = qq;
    }
    for (int t = 0; t < T; ++t)
      if (mq[t] >= 0) tclass[mq[t]] = tlab[t];
  }
  __syncthreads();
  if (q < T) a.match[((size_t)l * a.B + b) * T + q] = mq[q];
  // per-query terms (fp64): weight, weighted NLL, predicted-object count
  double w = 0.0, wnll = 0.0, card = 0.0;
  if (q < Q) {
    const int tc = tclass[q];
    w = tc == C - 1 ? (double)a.eos_coef : 1.0;
    wnll = w * -((double)lg[q * C + tc] - (double)mx - (double)lse);
    card = amax[q] != C - 1 ? 1.0 : 0.0;
  }
  // per-target terms: top-1 hit of the matched query and its point's three sums
  double hit = 0.0, l1 = 0.0, unc = 0.0, dif = 0.0;
  if (q < T && mq[q] >= 0) {
    const int qq = mq[q];
    hit = amax[qq] == tlab[q] ? 1.0 : 0.0;
    for (int d = 0; d < 2; ++d) {
      const float df = pt[2 * qq + d] - tp[2 * q + d];
      const float sg = ls ? ls[2 * qq + d] : 0.f;
      l1 += (double)fabsf(df);
      unc += (double)(fabsf(df) * expf(-sg) + 0.5f * sg);
      dif += (double)df;
    }
  }
  // wave reductions in lane order (xor tree: deterministic)
  double vals[7] = {w, wnll, card, hit, l1, unc, dif};
  for (int k = 0; k < 7; ++k) {
    double x = vals[k];
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    vals[k] = x;
  }
  if (q == 0) {
    double* p = a.partial + ((size_t)l * a.B + b) * NPART;
    vals[2] = fabs(vals[2] - (double)T);
    for (int k = 0; k < 7; ++k) p[k] = vals[k];
  }
}

__global__ __launch_bounds__(64) void criterion_sigma_reduce_kernel(CritSigmaArgs a) {
  const int l = blockIdx.x;
  if (threadIdx.x != 0) return;
  double s[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int b = 0; b < a.B; ++b)
    for (int k = 0; k < 7; ++k) s[k] += a.partial[((size_t)l * a.B + b) * NPART + k];
  double* o = a.losses + (size_t)l * 6;
  o[0] = s[1] / s[0];                                    // loss_ce
  o[1] = 100.0 - 100.0 * s[3] / ((double)a.B * a.T);     // class_error
  o[2] = s[2] / a.B;                                     // cardinality_error
  o[3] = s[4] / a.num_boxes;                             // loss_bbox (points)
  o[4] = s[5] / a.num_boxes;                             // loss_bbox (points_uncert)
  o[5] = s[6];                                           // points_different
}

}  // namespace

size_t spe_criterion_sigma_partial_bytes(int L, int B) { return (size_t)L * B * NPART * sizeof(double); }

int spe_launch_criterion_sigma(const CritSigmaArgs& a, hipStream_t s) {
  if (a.L <= 0 || a.B <= 0) return 0;
  if (a.Q < 1 || a.Q > QMAX || a.T < 1 || a.T > TMAX || a.T > a.Q || a.C < 2 || a.C > CMAX || !a.partial) return -5;
  hipLaunchKernelGGL(criterion_sigma_match_kernel, dim3(a.L * a.B), dim3(64), 0, s, a);
  hipLaunchKernelGGL(criterion_sigma_reduce_kernel, dim3(a.L), dim3(64), 0, s, a);
  return (int)hipGetLastError();
}
