// C entry points of the native runtime outside the model's forward pass (include/spe.h): the set
// criterion, ensemble fusion, pre- and post-processing, the batched solver, its self-assessment, the pose
// covariance, the calibration records, the landmark reconstruction and the SPEED score.  No allocation or synchronisation happens
// inside spe_pnp_batch / spe_pnp_exhaustive / spe_speed_score once the per-stream scratch has its size,
// so a caller may capture them into a hipGraph.
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <tuple>

#include "launch.h"
#include "model_state.h"
#include "spe_pnp.h"

#define fail spe_fail

// Device scratch of the solver's RANSAC hypothesis records and the criterion's per-image partial
// sums: one buffer per (device, stream, kind), grown on demand and kept for the process lifetime,
// so steady-state calls allocate nothing (a first call with a larger batch allocates and must
// therefore happen outside graph capture).  Keying by stream is what makes concurrent calls safe:
// calls on one stream are ordered by the stream, calls on different streams never share records.
// A stream handle that is destroyed while its work is pending and then reissued by the runtime
// would inherit the buffer; callers keep solver streams alive for as long as they use them.
static void* stream_scratch(hipStream_t stream, int kind, size_t bytes) {
  static std::mutex mu;
  static std::map<std::tuple<int, hipStream_t, int>, std::pair<void*, size_t>> bufs;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> g(mu);
  auto& e = bufs[std::make_tuple(dev, stream, kind)];
  if (e.second < bytes) {
    // the old buffer may still be read by work queued on this stream: free it in stream order
    if (e.first) {
      if (hipStreamSynchronize(stream) != hipSuccess) return nullptr;
      (void)hipFree(e.first);
    }
    e.first = nullptr;
    e.second = 0;
    if (hipMalloc(&e.first, bytes) != hipSuccess) return nullptr;
    e.second = bytes;
  }
  return e.first;
}
enum { SCRATCH_CRITERION = 0, SCRATCH_HYP = 1, SCRATCH_CRITERION_SIGMA = 2, SCRATCH_EXH = 3 };

extern "C" {

int spe_criterion(void* stream, const float* logits, const float* points, const int32_t* tgt_labels,
                  const float* tgt_points, int layers, int batch, int num_queries, int num_classes, int num_targets,
                  float cost_class, float cost_pts, float eos_coef, double num_points, int32_t* match, double* losses) {
  if (!logits || !points || !tgt_labels || !tgt_points || !match || !losses || layers < 1 || batch < 0 ||
      num_queries < 1 || num_queries > 64 || num_targets < 1 || num_targets > 32 || num_targets > num_queries ||
      num_classes < 2 || num_classes > 32 || !(num_points > 0))
    return fail(SPE_E_ARG, "bad argument");
  CritArgs a{logits, points, tgt_labels, tgt_points, layers, batch, num_queries, num_classes, num_targets,
             cost_class, cost_pts, eos_coef, num_points, match, nullptr, losses};
  if (batch > 0) {
    a.partial = (double*)stream_scratch((hipStream_t)stream, SCRATCH_CRITERION, (size_t)layers * batch * 5 * sizeof(double));
    if (!a.partial) return fail(SPE_E_LAUNCH, "criterion scratch allocation failed");
  }
  CK(spe_launch_criterion(a, (hipStream_t)stream));
  return 0;
}

int spe_criterion_sigma(void* stream, const float* logits, const float* points, const float* log_sigmas,
                        const int32_t* layer_has_sigma, const int32_t* tgt_labels, const float* tgt_points,
                        int layers, int batch, int num_queries, int num_classes, int num_targets,
                        float cost_class, float cost_bbox, int sigmoid_cost, float eos_coef, double num_boxes,
                        int32_t* match, double* losses) {
  if (!logits || !points || (log_sigmas && !layer_has_sigma) || !tgt_labels || !tgt_points || !match || !losses ||
      layers < 1 || batch < 0 || num_queries < 1 || num_queries > 64 || num_targets < 1 || num_targets > 32 ||
      num_targets > num_queries || num_classes < 2 || num_classes > 64 || !(num_boxes > 0))
    return fail(SPE_E_ARG, "bad argument");
  CritSigmaArgs a{logits, points, log_sigmas, layer_has_sigma, tgt_labels, tgt_points, layers, batch, num_queries,
                  num_classes, num_targets, cost_class, cost_bbox, sigmoid_cost != 0, eos_coef, num_boxes, match,
                  nullptr, losses};
  if (batch > 0) {
    a.partial = (double*)stream_scratch((hipStream_t)stream, SCRATCH_CRITERION_SIGMA,
                                        spe_criterion_sigma_partial_bytes(layers, batch));
    if (!a.partial) return fail(SPE_E_LAUNCH, "criterion scratch allocation failed");
  }
  CK(spe_launch_criterion_sigma(a, (hipStream_t)stream));
  return 0;
}

int spe_ensemble_fuse(void* stream, const float* points_px, const float* probs, int models, int batch,
                      int num_queries, int num_classes, float* fused_points, float* fused_probs) {
  if (!points_px || !probs || !fused_points || !fused_probs || models < 1 || batch < 0 || num_queries < 1 ||
      num_classes < 2 || num_classes > 17 || (int64_t)models * num_queries > 256)
    return fail(SPE_E_ARG, "bad argument");
  EnsembleArgs a{points_px, probs, models, batch, num_queries, num_classes, fused_points, fused_probs};
  CK(spe_launch_ensemble_fuse(a, (hipStream_t)stream));
  return 0;
}

int spe_ensemble_fuse_sigma(void* stream, const float* points_px, const float* probs, const float* sigmas,
                            const float* sigma_scale, int models, int batch, int num_queries, int num_classes,
                            float sigma_floor, float gate, float* fused_points, float* fused_probs,
                            float* fused_sigmas, int32_t* n_pooled, int32_t* n_kept) {
  if (!points_px || !probs || !sigmas || !fused_points || !fused_probs || !fused_sigmas || !n_pooled || !n_kept ||
      models < 1 || models > 16 || batch < 1 || num_queries < 1 || num_classes < 2 || num_classes > 17 ||
      (int64_t)models * num_queries > 256)
    return fail(SPE_E_ARG, "bad argument");
  if (!(gate > 0)) return fail(SPE_E_ARG, "gate must be positive");
  if (!(sigma_floor > 0) || !(sigma_floor < INFINITY)) return fail(SPE_E_ARG, "sigma_floor must be positive and finite");
  EnsembleSigmaArgs a{points_px, probs, sigmas, sigma_scale, models, batch, num_queries, num_classes, sigma_floor,
                      gate, fused_points, fused_probs, fused_sigmas, n_pooled, n_kept};
  CK(spe_launch_ensemble_fuse_sigma(a, (hipStream_t)stream));
  return 0;
}

// the lens kernels move points and sigmas as float2
static bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

int spe_undistort_points(void* stream, const float* points_px, const float* sigmas, const float* sigma_scale,
                         int batch, int num_queries, const double* K, const double* dist, int iters,
                         float* points_ideal, float* sigmas_ideal, uint8_t* status) {
  if (!points_px || !K || !dist || !points_ideal || batch < 1 || num_queries < 1 ||
      (int64_t)batch * num_queries > ((int64_t)1 << 30))
    return fail(SPE_E_ARG, "bad argument");
  if (iters < 1 || iters > 64) return fail(SPE_E_ARG, "iters must be in [1, 64]");
  if (sigmas_ideal && !sigmas) return fail(SPE_E_ARG, "sigmas_ideal needs sigmas");
  if (!aligned8(points_px) || !aligned8(sigmas) || !aligned8(points_ideal) || !aligned8(sigmas_ideal))
    return fail(SPE_E_ARG, "points and sigmas must be 8-byte aligned");
  LensArgs a{points_px, sigmas, sigma_scale, (size_t)batch * num_queries, num_queries, K, dist, iters,
             points_ideal, sigmas_ideal, status};
  CK(spe_launch_undistort_points(a, (hipStream_t)stream));
  return 0;
}

int spe_distort_points(void* stream, const float* points_ideal, int batch, int num_queries, const double* K,
                       const double* dist, float* points_px) {
  if (!points_ideal || !K || !dist || !points_px || batch < 1 || num_queries < 1 ||
      (int64_t)batch * num_queries > ((int64_t)1 << 30))
    return fail(SPE_E_ARG, "bad argument");
  if (!aligned8(points_ideal) || !aligned8(points_px)) return fail(SPE_E_ARG, "points must be 8-byte aligned");
  LensArgs a{points_ideal, nullptr, nullptr, (size_t)batch * num_queries, num_queries, K, dist, 1, points_px,
             nullptr, nullptr};
  CK(spe_launch_distort_points(a, (hipStream_t)stream));
  return 0;
}

int spe_preprocess(void* stream, const uint8_t* frames, int batch, int height, int width, int channels,
                   const double* bbox_xxyy, int size, float* images, float* clip_bbox, int32_t* status) {
  if (!frames || !bbox_xxyy || !images || !clip_bbox || batch < 0 || height <= 0 || width <= 0 || size <= 0 ||
      (channels != 1 && channels != 3))
    return fail(SPE_E_ARG, "bad argument");
  CK(spe_launch_preprocess(frames, batch, height, width, channels, bbox_xxyy, size, images, clip_bbox, status,
                           (hipStream_t)stream));
  return 0;
}

int spe_preprocess_submission(void* stream, const uint8_t* frames, int batch, int height, int width, int channels,
                              const double* bbox_xxyy, int size, float* images, uint8_t* crops_u8, float* clip_bbox,
                              int32_t* status) {
  if (!frames || !bbox_xxyy || (!images && !crops_u8) || !clip_bbox || batch < 0 || height <= 0 || width <= 0 ||
      size <= 0 || (channels != 1 && channels != 3))
    return fail(SPE_E_ARG, "bad argument");
  CK(spe_launch_preprocess_submission(frames, batch, height, width, channels, bbox_xxyy, size, images, crops_u8,
                                      clip_bbox, status, (hipStream_t)stream));
  return 0;
}

int spe_postprocess(void* stream, const float* logits, const float* points, const float* clip_bbox, int B, int Q,
                    float* probs, float* points_px) {
  if (!logits || !points || !clip_bbox || !probs || !points_px || B < 0 || Q <= 0) return fail(SPE_E_ARG, "bad argument");
  CK(spe_launch_postprocess(logits, points, clip_bbox, B, Q, probs, points_px, (hipStream_t)stream));
  return 0;
}

int spe_pnp_batch(void* stream, const float* points_px, const float* probs, const float* sigmas, int B, int Q, int C,
                  const double* K, const double* world, int mode, float repro, int ransac_iters, double confidence,
                  float* quat, double* tvec, double* rvec, int32_t* status, int32_t* n_corr, int32_t* corr_label,
                  uint32_t* inlier_mask, const float* repro_per_image) {
  if (!points_px || !probs || !K || !world || !quat || !tvec || B < 0 || Q <= 0 || Q > 64 || C < 2 || C > 17)
    return fail(SPE_E_ARG, "bad argument");
  if (mode < SPE_PNP_EPNP || mode > SPE_PNP_EPNP_CERES) return fail(SPE_E_ARG, "bad solver mode");
  if (ransac_iters < 1 || ransac_iters > 255 || !(confidence > 0 && confidence < 1))
    return fail(SPE_E_ARG, "ransac_iters must be in [1,255], confidence in (0,1)");
  PnpArgs a{};
  a.points = points_px; a.probs = probs; a.sigmas = sigmas;
  a.B = B; a.Q = Q; a.C = C; a.K = K; a.world = world; a.mode = mode; a.repro = repro;
  a.repro_img = repro_per_image;
  a.ransac_iters = ransac_iters; a.confidence = confidence;
  a.quat = quat; a.tvec = tvec; a.rvec = rvec; a.status = status; a.n_corr = n_corr;
  a.corr_label = corr_label; a.inlier_mask = inlier_mask;
  if (mode == SPE_PNP_EPNP_RANSAC_SIGMA && B > 0) {
    a.hyp = (HypRec*)stream_scratch((hipStream_t)stream, SCRATCH_HYP, (size_t)B * ransac_iters * sizeof(HypRec));
    a.hyp_stride = ransac_iters;
    if (!a.hyp) return fail(SPE_E_LAUNCH, "hypothesis scratch allocation failed");
  }
  CK(spe_launch_pnp(a, (hipStream_t)stream));
  return 0;
}

static int pnp_exhaustive(void* stream, const float* points_px, const float* probs, const float* sigmas, int B, int Q,
                          int C, const double* K, const double* world, float repro, int topk, float* quat, double* tvec,
                          double* rvec, int32_t* status, int32_t* n_corr, int32_t* corr_label, uint32_t* inlier_mask,
                          const float* repro_per_image, int32_t* cand_index, float* repro_final, int stages) {
  if (!points_px || !probs || !K || !world || !quat || !tvec || B < 0 || Q <= 0 || Q > 64 || C < 2 || C > 17)
    return fail(SPE_E_ARG, "bad argument");
  if (topk < 1 || topk > 64) return fail(SPE_E_ARG, "topk must be in [1,64]");
  if (stages < 1 || stages > 3) return fail(SPE_E_ARG, "bad stage mask");
  if (B == 0) return 0;
  PnpArgs a{};
  a.points = points_px; a.probs = probs; a.sigmas = sigmas;
  a.B = B; a.Q = Q; a.C = C; a.K = K; a.world = world; a.mode = SPE_PNP_EXHAUSTIVE; a.repro = repro;
  a.repro_img = repro_per_image;
  a.quat = quat; a.tvec = tvec; a.rvec = rvec; a.status = status; a.n_corr = n_corr;
  a.corr_label = corr_label; a.inlier_mask = inlier_mask;
  ExhRec* rec = (ExhRec*)stream_scratch((hipStream_t)stream, SCRATCH_EXH,
                                        (size_t)B * spe_pnp_exhaustive_subsets(C) * sizeof(ExhRec));
  if (!rec) return fail(SPE_E_LAUNCH, "hypothesis scratch allocation failed");
  CK(spe_launch_pnp_exhaustive(a, rec, topk, cand_index, repro_final, stages, (hipStream_t)stream));
  return 0;
}

int spe_pnp_exhaustive(void* stream, const float* points_px, const float* probs, const float* sigmas, int B, int Q, int C,
                       const double* K, const double* world, float repro, int topk, float* quat, double* tvec,
                       double* rvec, int32_t* status, int32_t* n_corr, int32_t* corr_label, uint32_t* inlier_mask,
                       const float* repro_per_image, int32_t* cand_index, float* repro_final) {
  return pnp_exhaustive(stream, points_px, probs, sigmas, B, Q, C, K, world, repro, topk, quat, tvec, rvec, status,
                        n_corr, corr_label, inlier_mask, repro_per_image, cand_index, repro_final, 3);
}

int spe_debug_pnp_exhaustive_stages(void* stream, const float* points_px, const float* probs, const float* sigmas, int B,
                                    int Q, int C, const double* K, const double* world, float repro, int topk,
                                    float* quat, double* tvec, double* rvec, int32_t* status, int32_t* n_corr,
                                    int32_t* corr_label, uint32_t* inlier_mask, const float* repro_per_image,
                                    int32_t* cand_index, float* repro_final, int stages) {
  return pnp_exhaustive(stream, points_px, probs, sigmas, B, Q, C, K, world, repro, topk, quat, tvec, rvec, status,
                        n_corr, corr_label, inlier_mask, repro_per_image, cand_index, repro_final, stages);
}

int spe_self_assess(void* stream, const float* probs, const float* sigmas, const int32_t* status,
                    const int32_t* corr_label, const uint32_t* inlier_mask, int B, int Q, int C, float score_th,
                    float sigma_th, int min_inliers, float* mean_sigma, int32_t* n_confident, uint8_t* reliable) {
  if (!probs || !sigmas || !status || !corr_label || !inlier_mask || !mean_sigma || !n_confident || !reliable || B < 0 ||
      Q <= 0 || Q > 64 || C < 2 || C > 17 || min_inliers < 0)
    return fail(SPE_E_ARG, "bad argument");
  SelfAssessArgs a{probs, sigmas, status, corr_label, inlier_mask, B, Q, C, score_th, sigma_th, min_inliers,
                   mean_sigma, n_confident, reliable};
  CK(spe_launch_self_assess(a, (hipStream_t)stream));
  return 0;
}

int spe_pose_covariance(void* stream, const float* probs, const float* sigmas, const float* sigma_scale,
                        const int32_t* status, const int32_t* corr_label, const uint32_t* inlier_mask,
                        const double* rvec, const double* tvec, int B, int Q, int C, const double* K,
                        const double* world, float sigma_floor, double* cov, float* sigma_rot, double* sigma_t,
                        float* pred_score, int32_t* cov_status) {
  if (!probs || !sigmas || !status || !corr_label || !inlier_mask || !rvec || !tvec || !K || !world || !cov ||
      !sigma_rot || !sigma_t || !pred_score || !cov_status || B < 1 || Q <= 0 || Q > 64 || C < 2 || C > 17)
    return fail(SPE_E_ARG, "bad argument");
  if (!(sigma_floor > 0) || !(sigma_floor < INFINITY)) return fail(SPE_E_ARG, "sigma_floor must be positive and finite");
  PoseCovArgs a{probs, sigmas, sigma_scale, status, corr_label, inlier_mask, rvec, tvec, B, Q, C, K, world,
                sigma_floor, cov, sigma_rot, sigma_t, pred_score, cov_status};
  CK(spe_launch_pose_cov(a, (hipStream_t)stream));
  return 0;
}

int spe_calibration_records(void* stream, const float* points_px, const float* probs, const float* sigmas,
                            const float* sigma_scale, float sigma_floor, const int32_t* status,
                            const int32_t* corr_label, const uint32_t* inlier_mask, const double* rvec,
                            const double* tvec, const double* q_gt, const double* t_gt, const double* cov,
                            const int32_t* cov_status, int B, int Q, int C, const double* K, const double* world,
                            double sigma_gain, double* delta, double* nees, double* z, uint8_t* kp_flags,
                            int32_t* calib_status) {
  if (!points_px || !probs || !sigmas || !status || !corr_label || !inlier_mask || !rvec || !tvec || !q_gt || !t_gt ||
      !cov || !cov_status || !K || !world || !delta || !nees || !z || !kp_flags || !calib_status || B < 1 || Q <= 0 ||
      Q > 64 || C < 2 || C > 17)
    return fail(SPE_E_ARG, "bad argument");
  if (!(sigma_floor > 0) || !(sigma_floor < INFINITY)) return fail(SPE_E_ARG, "sigma_floor must be positive and finite");
  if (!(sigma_gain > 0) || !(sigma_gain < (double)INFINITY)) return fail(SPE_E_ARG, "sigma_gain must be positive and finite");
  CalibArgs a{points_px, probs, sigmas, sigma_scale, sigma_floor, status, corr_label, inlier_mask, rvec, tvec, q_gt,
              t_gt, cov, cov_status, B, Q, C, K, world, sigma_gain, delta, nees, z, kp_flags, calib_status};
  CK(spe_launch_calib_records(a, (hipStream_t)stream));
  return 0;
}

int spe_landmark_observations(void* stream, const float* points_px, const float* probs, const float* sigmas,
                              const float* sigma_scale, int batch, int num_queries, int num_classes,
                              int64_t row_offset, double* obs_px, double* obs_sigma, uint8_t* obs_valid) {
  if (!points_px || !probs || !obs_px || !obs_valid || batch < 1 || num_queries <= 0 || num_queries > 64 ||
      num_classes < 2 || num_classes > 17 || row_offset < 0)
    return fail(SPE_E_ARG, "bad argument");
  LandmarkObsArgs a{points_px, probs, sigmas, sigma_scale, batch, num_queries, num_classes, (size_t)row_offset,
                    obs_px, obs_sigma, obs_valid};
  CK(spe_launch_landmark_observations(a, (hipStream_t)stream));
  return 0;
}

int64_t spe_landmarks_scratch_bytes(int num_views, int num_landmarks) {
  return (int64_t)spe_landmarks_scratch_size(num_views, num_landmarks);
}

int spe_landmarks_solve(void* stream, const double* obs_px, const double* obs_sigma, const uint8_t* obs_valid,
                        const double* q_gt, const double* t_gt, int num_views, int num_landmarks, const double* K,
                        const double* world_init, int iterations, double huber, double sigma_floor,
                        double sigma_gain, double z_min, void* scratch, int64_t scratch_bytes, double* world,
                        double* cov, double* chi2, int32_t* n_used, double* rms_px, uint8_t* obs_flags,
                        int32_t* lm_status) {
  if (!obs_px || !obs_valid || !q_gt || !t_gt || !K || !scratch || !world || !cov || !chi2 || !n_used || !rms_px ||
      !obs_flags || !lm_status || num_views < 1 || num_landmarks < 1 || num_landmarks > 16)
    return fail(SPE_E_ARG, "bad argument");
  if (iterations < 0 || iterations > 64) return fail(SPE_E_ARG, "iterations must be in [0, 64]");
  if (!(sigma_floor > 0) || !(sigma_floor < (double)INFINITY)) return fail(SPE_E_ARG, "sigma_floor must be positive and finite");
  if (!(sigma_gain > 0) || !(sigma_gain < (double)INFINITY)) return fail(SPE_E_ARG, "sigma_gain must be positive and finite");
  if (((uintptr_t)scratch & 7) != 0 || scratch_bytes < spe_landmarks_scratch_bytes(num_views, num_landmarks))
    return fail(SPE_E_WORKSPACE, "scratch misaligned or below spe_landmarks_scratch_bytes");
  LandmarkArgs a{obs_px, obs_sigma, obs_valid, q_gt, t_gt, num_views, num_landmarks, K, world_init, iterations,
                 huber, sigma_floor, sigma_gain, z_min, scratch, world, cov, chi2, n_used, rms_px, obs_flags,
                 lm_status};
  CK(spe_launch_landmarks_solve(a, (hipStream_t)stream));
  return 0;
}

int spe_speed_score(void* stream, const float* quat, const double* tvec, const double* q_gt, const double* t_gt, int B,
                    double* s_t, double* s_q) {
  if (!quat || !tvec || !q_gt || !t_gt || !s_t || !s_q || B < 0) return fail(SPE_E_ARG, "bad argument");
  CK(spe_launch_score(quat, tvec, q_gt, t_gt, B, s_t, s_q, (hipStream_t)stream));
  return 0;
}

}  // extern "C"
