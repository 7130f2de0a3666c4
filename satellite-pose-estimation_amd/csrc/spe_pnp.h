// Pose-solver launcher interface (internal; public entry points are in include/spe.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spe.h"

// One EPnP-RANSAC hypothesis (pnp_hyp_kernel -> pnp_kernel)
struct HypRec {
  double rt[6];            // rvec, tvec
  uint32_t mask;           // float32 inlier set over the correspondences
  int good, ok, pad;
};

struct PnpArgs {
  const float* points;     // [B][Q][2] image px (PostProcess output)
  const float* probs;      // [B][Q][C] softmax probabilities
  const float* sigmas;     // [B][Q][2] or null
  int B, Q, C;
  const double* K;         // 3x3 row-major (device)
  const double* world;     // [C-1][3] landmarks (device)
  int mode;                // SPE_PNP_*
  float repro;             // RANSAC / inlier reprojection threshold (px)
  const float* repro_img;  // [B] per-image threshold replacing repro (EPnPCeresSolver's area rule) or null
  int ransac_iters;        // cv2 default 100
  double confidence;       // cv2 default 0.99
  float* quat;             // [B][4] (float32 values, mathutils)
  double* tvec;            // [B][3]
  double* rvec;            // [B][3] or null
  int32_t* status;         // [B] or null
  int32_t* n_corr;         // [B] or null
  int32_t* corr_label;     // [B][16] or null
  uint32_t* inlier_mask;   // [B] or null (bit i = correspondence i)
  HypRec* hyp;             // [B][hyp_stride] scratch for the EPnP-RANSAC hypotheses (sigma mode) or null
  int hyp_stride;
};
int spe_launch_pnp(const PnpArgs& a, hipStream_t s);

// One four-point EPnP hypothesis of the exhaustive solver (pnp_exh_hyp_kernel -> pnp_exh_refine_kernel)
struct ExhRec {
  double rt[6];            // rvec, tvec
  float err;               // float32 sum of the 4 squared reprojection errors; +inf: not finite, never selected
  int pad;
};
// records per image: C(C-1, 4), the subsets of a full set of landmarks
int spe_pnp_exhaustive_subsets(int C);
// SPE_PNP_EXHAUSTIVE on PnpArgs (mode, ransac_iters, confidence, hyp unused); rec: [B][spe_pnp_exhaustive_subsets(C)].
// stages: bit 0 the hypothesis kernel, bit 1 selection + refinement (3 = the solver).
int spe_launch_pnp_exhaustive(const PnpArgs& a, ExhRec* rec, int topk, int32_t* cand_index, float* repro_final,
                              int stages, hipStream_t s);

struct SelfAssessArgs {
  const float* probs;         // [B][Q][C]
  const float* sigmas;        // [B][Q][2]
  const int32_t* status;      // [B]     (pnp_kernel outputs)
  const int32_t* corr_label;  // [B][16]
  const uint32_t* inlier_mask;// [B]
  int B, Q, C;
  float score_th, sigma_th;
  int min_inliers;
  float* mean_sigma;          // [B]
  int32_t* n_confident;       // [B]
  uint8_t* reliable;          // [B]
};
int spe_launch_self_assess(const SelfAssessArgs& a, hipStream_t s);

// Pose covariance from the keypoint sigmas (include/spe.h spe_pose_covariance)
struct PoseCovArgs {
  const float* probs;         // [B][Q][C]
  const float* sigmas;        // [B][Q][2]
  const float* sigma_scale;   // [B][2] or null
  const int32_t* status;      // [B]     (solver outputs)
  const int32_t* corr_label;  // [B][16]
  const uint32_t* inlier_mask;// [B]
  const double* rvec;         // [B][3]
  const double* tvec;         // [B][3]
  int B, Q, C;
  const double* K;            // 3x3 row-major
  const double* world;        // [C-1][3]
  float sigma_floor;
  double* cov;                // [B][6][6]
  float* sigma_rot;           // [B]
  double* sigma_t;            // [B][3]
  float* pred_score;          // [B]
  int32_t* cov_status;        // [B]
};
int spe_launch_pose_cov(const PoseCovArgs& a, hipStream_t s);

// Calibration records against ground truth (include/spe.h spe_calibration_records; csrc/calib.hip)
struct CalibArgs {
  const float* points;        // [B][Q][2] px, the image the pose was solved in
  const float* probs;         // [B][Q][C]
  const float* sigmas;        // [B][Q][2]
  const float* sigma_scale;   // [B][2] or null
  float sigma_floor;
  const int32_t* status;      // [B]     (solver outputs)
  const int32_t* corr_label;  // [B][16]
  const uint32_t* inlier_mask;// [B]
  const double* rvec;         // [B][3]
  const double* tvec;         // [B][3]
  const double* q_gt;         // [B][4]
  const double* t_gt;         // [B][3]
  const double* cov;          // [B][6][6] (spe_pose_covariance)
  const int32_t* cov_status;  // [B]
  int B, Q, C;
  const double* K;            // 3x3 row-major
  const double* world;        // [C-1][3]
  double sigma_gain;
  double* delta;              // [B][6]
  double* nees;               // [B][3]
  double* z;                  // [B][C-1][2]
  uint8_t* kp_flags;          // [B][C-1]
  int32_t* calib_status;      // [B]
};
int spe_launch_calib_records(const CalibArgs& a, hipStream_t s);

// Landmark reconstruction from posed observations (include/spe.h spe_landmarks_solve; csrc/landmarks.hip)
struct LandmarkObsArgs {
  const float* points;        // [B][Q][2] px
  const float* probs;         // [B][Q][C]
  const float* sigmas;        // [B][Q][2] or null
  const float* sigma_scale;   // [B][2] or null
  int B, Q, C;
  size_t row_offset;          // image b is written at row row_offset + b
  double* obs_px;             // [rows][C-1][2]
  double* obs_sigma;          // [rows][C-1][2] or null
  uint8_t* obs_valid;         // [rows][C-1]
};
int spe_launch_landmark_observations(const LandmarkObsArgs& a, hipStream_t s);

struct LandmarkArgs {
  const double* obs_px;       // [N][L][2]
  const double* obs_sigma;    // [N][L][2] or null: 1 px
  const uint8_t* obs_valid;   // [N][L]
  const double* q_gt;         // [N][4]
  const double* t_gt;         // [N][3]
  int N, L;
  const double* K;            // 3x3 row-major
  const double* world_init;   // [L][3] or null
  int iterations;
  double huber, sigma_floor, sigma_gain, z_min;
  void* scratch;              // spe_landmarks_scratch_bytes(N, L)
  double* world;              // [L][3]
  double* cov;                // [L][3][3]
  double* chi2;               // [L]
  int32_t* n_used;            // [L]
  double* rms_px;             // [L]
  uint8_t* obs_flags;         // [N][L]
  int32_t* lm_status;         // [L]
};
size_t spe_landmarks_scratch_size(int N, int L);
int spe_launch_landmarks_solve(const LandmarkArgs& a, hipStream_t s);
int spe_launch_score(const float* quat, const double* tvec, const double* q_gt, const double* t_gt, int B,
                     double* s_t, double* s_q, hipStream_t s);
