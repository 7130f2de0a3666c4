/* spe.h — C ABI of the MI355X-native keypoint-set pose path (libspe.so).
 *
 * The reference (wwhitecyan/satellite-pose-estimation, REV/ = "Revisiting Monocular Satellite
 * Pose Estimation With Transformer") has no FFI layer: its seams are Python call signatures.
 * Each entry point below replaces one of them; the Python host package (spe/) binds them with
 * ctypes and keeps the reference's call surface.
 *
 * Conventions: plain pointers and sizes only; device pointers are caller-owned HIP device memory;
 * `stream` is a hipStream_t (NULL = default stream); no entry point allocates or synchronises
 * on the hot path (spe_forward / spe_pnp_batch / spe_speed_score are graph-capturable);
 * return 0 on success, a negative SPE_E_* code on argument errors, or a positive hipError_t.
 */
#ifndef SPE_H_
#define SPE_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPE_ABI_VERSION 9

enum {
  SPE_E_ARG = -1,        /* bad argument / size */
  SPE_E_STATE = -2,      /* model not finalized / already finalized */
  SPE_E_MISSING = -3,    /* a required parameter key was never set */
  SPE_E_KEY = -4,        /* unknown parameter key or wrong element count */
  SPE_E_WORKSPACE = -5,  /* workspace too small */
  SPE_E_LAUNCH = -6      /* kernel launch rejected its shapes */
};

/* BF16_: bf16 storage, bf16 MFMA with fp32 accumulation (throughput mode); F32_: fp32 storage,
 * exact-f32 MFMA (parity mode); F16_: fp16 attention operands (attn_dtype only); F32X3_: fp32
 * storage, split-bf16 MFMA (x = hi + lo, products hi.hi + hi.lo + lo.hi, fp32 accumulation):
 * the fast parity mode on the reference goldens; F32X6_: the accuracy-contract mode (<= 1e-4 of the exact-f32
 * mode on the bench's amplifying weights too): fp32 storage, every GEMM / convolution with
 * near-fp32 precision (x = hi + mid + lo in bf16, the six products of relative order >= 2^-16), the
 * encoder attention contractions as F32X3_, the decoder attention (whose 64x-sharpened cross-attention
 * amplifies operand error most) in exact f32; F32H3_ (round 5): F32X6_ with the backbone / encoder GEMMs and
 * convolutions as three fp16 MFMAs on a two-way fp16 split (x.s = hi + lo, fp16 RNE each, s a power of two:
 * per output channel for the weights, per tensor for the activations from the producer's max |x|),
 * products hi.hi + hi.lo + lo.hi -- F32X6_'s accuracy (2^-22-level operands) at half its MFMAs */
enum { SPE_DTYPE_BF16_ = 0, SPE_DTYPE_F32_ = 1, SPE_DTYPE_F16_ = 2, SPE_DTYPE_F32X3_ = 4, SPE_DTYPE_F32X6_ = 5,
       SPE_DTYPE_F32H3_ = 6 };

/* Solver modes.
 *  SPE_PNP_EPNP              cv2.solvePnPGeneric(EPNP) on all selected points
 *                            (UNC/utils/speed_eval_ceres.py:153-169) — BASELINE config 2
 *  SPE_PNP_RANSAC_P3P_LM     cv2.solvePnPRansac(P3P) + solvePnPGeneric(ITERATIVE) on inliers
 *                            (REV/utils/speed_eval.py:209-230) — BASELINE config 3
 *  SPE_PNP_EPNP_RANSAC_SIGMA cv2.solvePnPRansac(EPNP) + sigma-weighted Huber LM
 *                            (UNC/utils/speed_eval.py:332-420) — BASELINE config 4
 *  SPE_PNP_EPNP_LM           EPnP + solvePnPGeneric(ITERATIVE) on all points
 *  SPE_PNP_EPNP_CERES        UNC EPnPCeresSolver (UNC/utils/speed_eval_ceres.py:43-243): EPnP on all points,
 *                            inliers = reprojection error < the image's threshold (get_repro_th, :53-58),
 *                            sigma-weighted Huber(0.001) LM on the inliers (weights normalised over them),
 *                            the EPnP pose kept when the refined error sum over all points is larger
 *                            (:142-146); exactly one inlier raises IndexError there -> status NO_FG;
 *                            no inlier -> status OK with the EPnP pose (the reference's own control flow
 *                            builds an empty Ceres problem, tests/golden/solver_front_ref.npz), PARITY
 *                            UNPINNED in one point: whether OpenCV 4.4's undistortPoints accepts the
 *                            empty point set (a cv2.error there would make SpeedEval log a zero pose)
 *  SPE_PNP_EXHAUSTIVE        UNC PoseSolver.exhausive_pnp behind SimplePoseSolver.__call__
 *                            (UNC/utils/speed_eval_ceres.py:326-399, :465-522), through spe_pnp_exhaustive only
 *                            (spe_pnp_batch refuses it).  EPnP on every four-point subset of the selected
 *                            correspondences in itertools.combinations order; a hypothesis's error is the
 *                            float32 sum of its 4 squared reprojection errors (cv2's reprojectionError is the
 *                            RMSE of the same, only the order is used), +inf when pose or error is not finite.
 *                            The topk smallest are kept; the sort is STABLE, ties go to the lower subset index
 *                            (np.argsort's default quicksort is not: equal errors are unpinned there), +inf
 *                            records are never kept.  Walking them in order with th = the image's threshold:
 *                            float32 errors of all points (epnp_init's arithmetic), inliers err < th; fewer
 *                            than 4 -> th += 5 (carried to later candidates) and the next one; else the
 *                            sigma-weighted Huber(0.001) LM on the inliers, weights normalised over them, the
 *                            unrefined pose kept when the refined error sum over all points is larger; the
 *                            candidate with the smallest sum (< 100000, the first of equals) wins.  The walk
 *                            repeats until a pass had a candidate with 4 inliers; th after s failures is
 *                            th0 + 5 s in fp64, and passes that cannot succeed are skipped arithmetically.
 *                            Status UNPINNED (zero pose) where the reference never returns: no finite
 *                            hypothesis, no kept candidate with 4 finite errors, or every qualifying
 *                            candidate's sum >= 100000 or NaN.  PARITY UNPINNED: cv2 is absent here (EPnP, the
 *                            projection and Rodrigues are the oracle's restatements), and the reference's call
 *                            ceres_pnp(inlier_wld, inlier_obj, r_, t_) (:382) lacks the sigma argument of its
 *                            own definition (:172), so it raises TypeError as written; the sigma rule above
 *                            (the selected sigmas, or unit weights without a sigma input) is this project's
 *                            reading, EPnPCeresSolver's.
 * SPE_PNP_EPNP's inlier_mask is epnp_init's set, reprojection error < repro (:163-166). */
enum { SPE_PNP_EPNP = 0, SPE_PNP_RANSAC_P3P_LM = 1, SPE_PNP_EPNP_RANSAC_SIGMA = 2, SPE_PNP_EPNP_LM = 3,
       SPE_PNP_EPNP_CERES = 4, SPE_PNP_EXHAUSTIVE = 5 };

/* Per-image solver status (reference exception mapping, REV/datasets/speed.py:355-363).
 *  OK              pose solved
 *  NO_FG           no foreground label -> IndexError in the reference -> zero pose
 *  CV_ERROR        fewer than 4 correspondences -> cv2.error (CV_Assert npoints >= 4) -> zero pose
 *  RANSAC_FALLBACK no consensus: the reference keeps the rvec/tvec of the last RANSAC hypothesis
 *                  (OpenCV's callback shares them) and skips refinement; same here
 *  UNPINNED        behaviour OpenCV leaves uninitialised (e.g. P3P failure on exactly 4 points);
 *                  defined here as a zero pose */
enum { SPE_PNP_OK = 0, SPE_PNP_NO_FG = 1, SPE_PNP_CV_ERROR = 2, SPE_PNP_RANSAC_FALLBACK = 3, SPE_PNP_UNPINNED = 4 };

typedef struct spe_model spe_model;

/* Mirrors the argparse fields build_model(args) reads (REV/main.py:90-187). */
typedef struct {
  int input_size;       /* --input_size (416) */
  int num_queries;      /* --num_queries (11) */
  int enc_layers;       /* --enc_layers (6) */
  int dec_layers;       /* --dec_layers (6) */
  int hidden_dim;       /* --hidden_dim (256; only 256 supported) */
  int nheads;           /* --nheads (8; head_dim must be 32) */
  int dim_feedforward;  /* --dim_feedforward (2048) */
  int sigma_head;       /* 1: UNC-style sigma head (sigma_embed.layers.*) */
  int dtype;            /* SPE_DTYPE_BF16_ (bf16 storage, fp32 accumulate), SPE_DTYPE_F32_, _F32X3_, _F32X6_ or _F32H3_ */
  int attn_dtype;       /* encoder self-attention operands (q, k, V^T): 0 = as dtype; SPE_DTYPE_F16_ =
                         * fp16 (bf16 models only; BASELINE config 5's "fp16 MFMA attention") */
} spe_model_config;

typedef struct {
  float* logits;          /* [B,Q,12] pred_logits (required) */
  float* points;          /* [B,Q,2]  pred_points, sigmoid, crop-normalised (required) */
  const float* clip_bbox; /* [B,4] x1,y1,x2,y2 (nullable) -> fused PostProcess */
  float* probs;           /* [B,Q,12] softmax(pred_logits) (nullable, needs clip_bbox) */
  float* points_px;       /* [B,Q,2]  image-pixel points (nullable, needs clip_bbox) */
  float* log_sigmas;      /* [B,Q,2]  sigma head raw output (nullable) */
  float* sigmas;          /* [B,Q,2]  exp(log_sigmas) (nullable) */
  float* hs;              /* [B,Q,256] last decoder layer after decoder_norm (nullable) */
  float* aux_logits;      /* [dec_layers-1,B,Q,12] aux outputs (nullable; aux_loss=True, */
  float* aux_points;      /* [dec_layers-1,B,Q,2]   REV/models/detr_speed.py:88-99)       */
} spe_forward_outputs;

/* UNC RT-DETR keypoint model with the sigma head: RTDETR(PResNet-vd, HybridEncoder,
 * RTDETRTransformer) (UNC/src/zoo/rtdetr/rtdetr.py:20-38, UNC/nn/backbone/presnet.py:156-265,
 * UNC/src/zoo/rtdetr/hybrid_encoder.py:196-401, UNC/src/zoo/rtdetr/rtdetr_decoder.py:372-710) as
 * the speed configs build it (UNC/configs/rtdetr_speed/rtdetr_r{18,50}vd_6x_speed_kl_*.yml). */
/* spe_rtdetr_config.depth value that selects MobileNetV3_Large (UNC/nn/backbone/mobilenetv3.py:123-225,
 * UNC/configs/rtdetr_speed/rtdetr_mobilenetv3_6x_speed_*.yml) instead of a PResNet depth.  That
 * backbone resizes its stem output to a hard-coded 64 x 64 before the stride-8 / 16 branch, so its three
 * maps are the stride 8 / 16 / 32 levels only at input_size 256: spe_rtdetr_create refuses every other
 * size (SPE_E_ARG), as the reference's own hybrid encoder does.  Its never-called linear3 / bn3
 * parameters are part of the key space (accepted and ignored). */
#define SPE_RTDETR_MBV3_LARGE 1003
/* spe_rtdetr_config.depth value that selects GhostNetV2 (UNC/nn/backbone/ghostnetv2.py:286-441,
 * UNC/configs/rtdetr_speed/include/rtdetr_ghostnetv2.yml).  It resizes its raw stem output to the same
 * hard-coded 64 x 64, so it too is accepted at input_size 256 only (SPE_E_ARG otherwise).  Its never-called
 * conv_head / classifier parameters are part of the key space (accepted and ignored). */
#define SPE_RTDETR_GHOSTNETV2 1004
/* spe_rtdetr_config.depth value that selects MobileNetV3_Small (UNC/nn/backbone/mobilenetv3.py:228-320, the
 * commented alternative of UNC/configs/rtdetr_speed/include/rtdetr_mobilenet.yml): 11 blocks, block 0 at the
 * full stem resolution with squeeze-excite and a depthwise-only skip, Conv1 / Conv2 bare convolutions.  The
 * same hard-coded 64 x 64 resize: input_size 256 only (SPE_E_ARG otherwise).  Its never-called linear3 / bn3
 * parameters are part of the key space (accepted and ignored).  Environment: SPE_MBS_ENTRY=0 runs block 0
 * launch by launch instead of through the fused entry kernel (read once per process). */
#define SPE_RTDETR_MBV3_SMALL 1005

typedef struct {
  int depth;            /* backbone selector: 18 (BasicBlock) or 50 (BottleNeck) = PResNet variant d of that
                         * depth; SPE_RTDETR_MBV3_LARGE = MobileNetV3_Large; SPE_RTDETR_GHOSTNETV2 = GhostNetV2;
                         * SPE_RTDETR_MBV3_SMALL = MobileNetV3_Small */
  int input_size;       /* eval_spatial_size (256); multiple of 32; MobileNetV3_Large / _Small / GhostNetV2: 256 only */
  int num_queries;      /* RTDETRTransformer.num_queries (30), <= 64 */
  int dec_layers;       /* num_decoder_layers (3) */
  int enc_ff;           /* HybridEncoder.dim_feedforward (1024, GELU) */
  int dec_ff;           /* RTDETRTransformer.dim_feedforward (1024, ReLU) */
  int csp_hidden;       /* CSPRepLayer hidden channels = 256 * expansion (128 for expansion 0.5) */
  int num_classes;      /* 11 (+1 no-object logit) */
  int dtype;            /* SPE_DTYPE_BF16_ or SPE_DTYPE_F32_ */
} spe_rtdetr_config;

typedef struct {
  float* logits;          /* [B,Q,C+1] pred_logits of the last decoder layer (required) */
  float* points;          /* [B,Q,2]   pred_pts, refined reference points, crop-normalised (required) */
  float* log_sigmas;      /* [B,Q,2]   pred_sigmas (raw sigma head, repeated to 2) (nullable) */
  const float* clip_bbox; /* [B,4] (nullable) -> fused RTDETRPostProcessor: */
  float* probs;           /*   [B,Q,C+1] softmax (rtdetr_postprocessor.py:44-76) */
  float* points_px;       /*   [B,Q,2] image pixels */
  float* sigmas;          /*   [B,Q,2] exp(pred_sigmas) */
  float* aux_logits;      /* [L-1,B,Q,C+1] earlier decoder layers (nullable; aux_outputs) */
  float* aux_points;      /* [L-1,B,Q,2] */
  float* aux_log_sigmas;  /* [L-1,B,Q,2] */
  float* enc_logits;      /* [B,Q,C+1] encoder top-k logits (nullable; last aux_outputs entry) */
  float* enc_points;      /* [B,Q,2]   sigmoid(enc_bbox_head + anchors) of the selected tokens */
  int32_t* topk;          /* [B,Q] selected encoder tokens, descending score (nullable) */
  float* hs;              /* [B,Q,256] last decoder layer output, the heads' input (nullable) */
} spe_rtdetr_outputs;

/* Create an RT-DETR model handle.  The lifecycle entry points of spe_model (set_param with the
 * reference's state_dict keys, num_params / param_name, finalize, workspace_bytes, destroy,
 * profile_*) apply to it unchanged; BatchNorm2d num_batches_tracked buffers are not parameters. */
int spe_rtdetr_create(const spe_rtdetr_config* cfg, spe_model** out);
/* RTDETR.forward in eval (+ RTDETRPostProcessor when clip_bbox is given).  images: device
 * [B,3,S,S] fp32, ImageNet-normalised (UNC/src/data/speed/speed_dataset.py:40-66). */
int spe_rtdetr_forward(spe_model* m, void* stream, const float* images, int batch, void* workspace,
                       int64_t workspace_bytes, const spe_rtdetr_outputs* out);

int spe_abi_version(void);
const char* spe_last_error(void);

/* Model lifecycle.  Replaces build_model(args) (REV/models/__init__.py:5-6) + load_state_dict
 * (REV/main.py:264-274): parameters are handed over by their reference state_dict key
 * (412 keys, e.g. "backbone.0.body.layer1.0.conv1.weight"), fp32, host memory. */
int spe_model_create(const spe_model_config* cfg, spe_model** out);
/* The same with the backbone named (additive, ABI 9; spe_model_create == SPE_BACKBONE_RESNET50_S8):
 *   SPE_BACKBONE_RESNET50_S8   Backbone8s, the stride-8 fusion neck (REV/models/backbone.py:105-149); 412 keys
 *   SPE_BACKBONE_RESNET50_S16  Backbone, ResNet-50 cut after layer3 (REV/models/backbone.py:57-102): no neck
 *                              parameters (408 keys), input_proj.weight [256][1024][1][1] straight on the
 *                              stride-16 map, T = (input_size / 16)^2 tokens
 * Everything after src (stages, u8 crops, attention maps, outputs) is the same for both. */
enum { SPE_BACKBONE_RESNET50_S8 = 0, SPE_BACKBONE_RESNET50_S16 = 1 };
int spe_model_create_backbone(const spe_model_config* cfg, int backbone, spe_model** out);
/* The same with a flags word, an OR of the bits below (additive, ABI 9; flags == 0 is spe_model_create_backbone):
 *   SPE_MODEL_PRE_NORM  the reference's --pre_norm transformer (REV/models/transformer.py forward_pre of both layer
 *                       classes): every LayerNorm in front of its sub-block, the encoder closed by
 *                       transformer.encoder.norm.{weight,bias} (two more keys, after the encoder layers': 414 / 410).
 *                       dtypes BF16_ (attn_dtype F16_ included), F32_, F32X3_ and F32X6_; F32H3_ is refused with
 *                       SPE_E_ARG (its activation-scale ledger rests on post-norm LayerNorm output bounds). */
/*   SPE_MODEL_GROUP_NORM  the reference's --bn group_bn backbone (REV/models/backbone.py:168-181): nn.GroupNorm(32, C),
 *                       eps 1e-5, in all 43 norm positions of the ResNet-50.  The keys are the reference's: every
 *                       ...bnN.weight / .bias and downsample.1.weight / .bias, no running_mean / running_var (326 keys
 *                       at stride 8, 322 at stride 16).  Nothing folds into a conv: every body conv runs bare and a
 *                       GroupNorm (groupnorm.hip: norm.gn.stats + norm.gn.apply) follows it.  Composes with both
 *                       backbones and with SPE_MODEL_PRE_NORM.  dtypes BF16_ (attn_dtype F16_ included), F32_, F32X3_
 *                       and F32X6_; F32H3_ is refused with SPE_E_ARG (its activation-scale ledger takes static
 *                       bounds from folded-BatchNorm weights; a GroupNorm output's scale depends on the data). */
/* (bit value 2 is not a flag and stays refused with SPE_E_ARG, as it was before SPE_MODEL_GROUP_NORM existed) */
enum { SPE_MODEL_PRE_NORM = 1, SPE_MODEL_GROUP_NORM = 4 };
int spe_model_create_flags(const spe_model_config* cfg, int backbone, int flags, spe_model** out);
void spe_model_destroy(spe_model* m);
int spe_model_set_param(spe_model* m, const char* key, const float* host_data, int64_t numel);
int spe_model_num_params(const spe_model* m);                 /* number of required keys */
const char* spe_model_param_name(const spe_model* m, int i);  /* i-th required key */
int spe_model_finalize(spe_model* m);  /* fold FrozenBN, pack NHWC/[N][K] weights, upload (current device) */
int64_t spe_model_workspace_bytes(const spe_model* m, int batch);

/* DETR.forward + PostProcess (REV/models/detr_speed.py:59-92,266-293).
 * images: device [B,3,S,S] fp32, ImageNet-normalised (REV/datasets/speed.py:25-41). */
int spe_forward(spe_model* m, void* stream, const float* images, int batch, void* workspace, int64_t workspace_bytes,
                const spe_forward_outputs* out);
/* The same pass split in two stages that may run on different streams: ENCODE = backbone +
 * neck + input_proj + encoder (images -> memory, kept in `workspace`), DECODE = decoder + heads +
 * PostProcess (memory in `workspace` -> out).  spe_forward == both stages in order.  A caller
 * that overlaps batch i's DECODE with batch i+1's ENCODE gives each in-flight batch its own
 * workspace. */
/* ENCODE itself splits in two: BACKBONE = backbone + neck + input_proj (images -> src in the
 * workspace) and TRANSFORMER = the encoder layers (src -> memory); ENCODE == BACKBONE followed by
 * TRANSFORMER.  A caller may run batch i's TRANSFORMER beside batch i+1's BACKBONE (the HBM-bound
 * convolutions beside the VALU-bound attention), each batch with its own workspace. */
enum { SPE_STAGE_ENCODE = 1, SPE_STAGE_DECODE = 2, SPE_STAGE_BACKBONE = 4, SPE_STAGE_TRANSFORMER = 8 };
int spe_forward_stages(spe_model* m, void* stream, const float* images, int batch, void* workspace,
                       int64_t workspace_bytes, const spe_forward_outputs* out, int stages);
/* The same stages fed with the 8-bit crops the validation transform produces before to_tensor +
 * Normalize (REV/datasets/speed.py:25-41, 209-233): crops = device [B][S][S][channels] u8 (channels 1:
 * grayscale, which Image.convert('RGB') replicates into three channels -- the SPEED frames -- or 3
 * RGB), normalised (u8 / 255 - mean) / std in fp32 inside the stem's input pack: bit-identical to
 * spe_forward_stages on the fp32 batch normalised that way, at a quarter (RGB) or a twelfth (gray) of
 * its bytes -- the form a host-side loader hands over PCIe (REV/engine.py:92 samples.to(device)).
 * (ABI 8 addition) */
int spe_forward_stages_u8(spe_model* m, void* stream, const uint8_t* crops, int channels, int batch, void* workspace,
                          int64_t workspace_bytes, const spe_forward_outputs* out, int stages);

/* spe_forward that also exports attention maps: what the reference's visualize_features.py hooks
 * (REV/visualize_features.py, output[1] of nn.MultiheadAttention: the probabilities averaged over the 8
 * heads) from transformer.encoder.layers[enc_layer].self_attn into enc_map, device fp32 [B,T,T] (T =
 * (input_size / 8)^2 tokens, row = query token, h * W + w order), and from
 * transformer.decoder.layers[dec_layer].multihead_attn into dec_map, device fp32 [B,Q,T].  The same
 * launch sequence as spe_forward (`out` is bit-identical) plus one launch of the map kernel (attn_map.hip)
 * per map, on the q / k operands the tapped layer's own attention kernel reads, in that mode's storage.
 * Either map may be NULL (that tap is skipped), not both.  Negative layer indices count from the end; the
 * reference's choice is enc_layer = -1, dec_layer = -2.  Graph-capturable like spe_forward.  Model dtypes
 * BF16_ (attn_dtype F16_ included) and F32_; SPE_E_ARG, before anything is launched, for the split-precision
 * modes (F32X3_ / F32X6_ / F32H3_: their operands live as split planes), an RT-DETR handle (that family's entry
 * is spe_rtdetr_forward_attention), a layer index out of range, both maps NULL. The workspace is spe_forward_attention_workspace_bytes (today equal to
 * spe_model_workspace_bytes: every served mode leaves q and k in the forward's own workspace). */
int64_t spe_forward_attention_workspace_bytes(const spe_model* m, int batch);
int spe_forward_attention(spe_model* m, void* stream, const float* images, int batch, void* workspace,
                          int64_t workspace_bytes, const spe_forward_outputs* out, int enc_layer, int dec_layer,
                          float* enc_map, float* dec_map);

/* spe_rtdetr_forward in stages, with the SPE_STAGE_* bits read for the RT-DETR model:
 *   BACKBONE     the backbone: images -> the stride 8 / 16 / 32 maps, kept in `workspace`
 *   TRANSFORMER  the HybridEncoder (input_proj, AIFI, FPN, PAN): the maps -> the three level outputs, kept
 *                in `workspace`
 *   ENCODE       BACKBONE followed by TRANSFORMER
 *   DECODE       the RTDETRTransformer, the heads and the fused RTDETRPostProcessor: `workspace` -> out
 * spe_rtdetr_forward == every stage in order: the same launches with the same results.  `stages` names
 * one stage or neighbours in that order (BACKBONE | DECODE without TRANSFORMER is refused); `out` may be NULL
 * when DECODE is not asked for, `images` when BACKBONE is not.
 * Staging contract: everything a later stage reads lies in `workspace`, and a forward writes device memory
 * nowhere else but `out` (the packed model is read-only after finalize).  Two batches in flight therefore
 * take two workspaces and share nothing writable; the stages of one batch are ordered by the caller
 * (one stream, or events between streams), and a workspace is free for the next batch once its DECODE is done.
 * Refusals, before any launch and in this order: a null handle / workspace or batch <= 0, a DETR handle
 * ("not an RT-DETR model"), a bad stage mask, BACKBONE without images / crops, DECODE without out /
 * out->logits / out->points, channels other than 1 or 3 (all SPE_E_ARG); a model not finalized
 * (SPE_E_STATE); a workspace below spe_model_workspace_bytes (SPE_E_WORKSPACE).  (ABI 9 addition) */
int spe_rtdetr_forward_stages(spe_model* m, void* stream, const float* images, int batch, void* workspace,
                              int64_t workspace_bytes, const spe_rtdetr_outputs* out, int stages);
/* The same stages fed with 8-bit crops, device [B][S][S][channels] u8 (channels 1: grayscale, replicated into
 * the three channels; 3: RGB) -- the pad-to-square crops of spe_preprocess_submission, which is UNC's
 * SpeedSubmission crop (UNC/src/data/speed/speed_dataset.py:59-168), or a loader's crops before to_tensor +
 * Normalize.  Each pixel is normalised (u8 / 255 - mean) / std in fp32 where the backbone first reads it (the
 * PResNet input pack, the MobileNetV3_Large / GhostNetV2 stem): bit-identical to spe_rtdetr_forward_stages on
 * the fp32 batch normalised that way. */
int spe_rtdetr_forward_stages_u8(spe_model* m, void* stream, const uint8_t* crops, int channels, int batch,
                                 void* workspace, int64_t workspace_bytes, const spe_rtdetr_outputs* out, int stages);

/* spe_rtdetr_forward that also exports attention maps (spe_forward_attention is the DETR entry and refuses an
 * RT-DETR handle; this one refuses a DETR handle).  All maps are device fp32, each nullable, not all four:
 *   enc_map      [B][T5][T5], T5 = (input_size / 32)^2: the AIFI layer's self-attention (encoder.encoder.0.layers.0.
 *                self_attn), the probabilities averaged over the 8 heads, row = query token, y * W + x order: the
 *                map kernel of spe_forward_attention (attn_map.hip) on the q / k the AIFI attention kernel reads
 *   dec_map      [B][Q][L], L = the memory tokens of one image in the reference's order (level-major: stride 8,
 *                16, 32; y * W_l + x inside a level): decoder.decoder.layers[dec_layer].cross_attn.  The multi-scale
 *                deformable attention forms no matrix: per head it reads levels x points = 12 bilinear samples with
 *                softmaxed weights w.  dec_map[b][q][t] = (1/8) sum_h sum_samples w . (the sample's bilinear weight
 *                on cell t), which is the matrix with cross_attn's sampled output = dec_map_h . value_h.  Corners off
 *                a level read grid_sample's zero padding and are dropped: a row sums to <= 1, the rest fell off the maps
 *   dec_loc      [B][Q][8][3][4][2]: the normalised sampling locations (x, y) in crop coordinates,
 *                reference point + offset / (W_l, H_l)
 *   dec_weights  [B][Q][8][3][4]: the weights w (softmax over a head's 12 samples)
 * The launch sequence of spe_rtdetr_forward (`out` is bit-identical) plus one launch of the map kernel for enc_map
 * and one of rt_deform_map (rtdetr.hip) after the tapped layer's msdeform; no host synchronisation, no
 * allocation.  Negative dec_layer counts from the end (-1: the last layer, whose points are the output).  The
 * workspace is spe_model_workspace_bytes.  Refusals, before any launch and in this order: a null handle /
 * workspace or batch <= 0, a DETR handle ("not an RT-DETR model"), null images / out / out->logits /
 * out->points, all four maps NULL, dec_layer out of range (all SPE_E_ARG); a model not finalized (SPE_E_STATE);
 * a workspace below spe_model_workspace_bytes (SPE_E_WORKSPACE).  (ABI 9 addition) */
int spe_rtdetr_forward_attention(spe_model* m, void* stream, const float* images, int batch, void* workspace,
                                 int64_t workspace_bytes, const spe_rtdetr_outputs* out, int dec_layer,
                                 float* enc_map, float* dec_map, float* dec_loc, float* dec_weights);

/* Validation input pipeline on the device (SpeedTrain.__getitem__ with train=False,
 * REV/datasets/speed.py:209-233): generate_clip_bbox_val (:246-258), Pillow crop,
 * A.Resize(S, S, cv2.INTER_CUBIC) (make_transforms(train=False), :295-299), F.to_tensor and
 * Normalize (:25-41).  frames: device uint8 [B,H,W] (channels = 1: grayscale, replicated to RGB
 * like Image.convert('RGB')) or [B,H,W,3]; bbox_xxyy: device fp64 [B,4] detector boxes;
 * images: fp32 [B,3,S,S] (spe_forward's input); clip_bbox: fp32 [B,4] (PostProcess's box);
 * status (nullable): [B] 0 ok, 1 empty crop (the reference raises; zeros written). */
int spe_preprocess(void* stream, const uint8_t* frames, int batch, int height, int width, int channels,
                   const double* bbox_xxyy, int size, float* images, float* clip_bbox, int32_t* status);

/* Submission input pipeline on the device (SpeedSubmission.__getitem__, REV/datasets/speed.py:92-160,
 * the dataset of gen_submission_single.py / gen_submission_multi.py): generate_clip_bbox (:92-108)
 * gives the integer square x1 = int(xc - s/2), y1 = int(yc - s/2), side = int(s), s = 1.2 x the
 * box's longer side (fp64, truncation towards zero), which is NOT clipped to the frame; the crop
 * (:126-144) is a side x side zero canvas holding the in-frame part of that square ("pad instead
 * of squeeze", 2020-12-14), then A.Resize(S, S, cv2.INTER_CUBIC), F.to_tensor and Normalize as in
 * spe_preprocess.  frames / bbox_xxyy as for spe_preprocess.  images (nullable): fp32 [B,3,S,S];
 * crops_u8 (nullable): uint8 [B,S,S,channels], the resized crop before to_tensor -- the input of
 * spe_forward_stages_u8; at least one of the two is required (else SPE_E_ARG).  clip_bbox: fp32
 * [B,4] = (x1, y1, x1 + side, y1 + side), PostProcess's box; it may be negative or extend past the
 * frame.  status (nullable): [B] 0 ok, 1 when side <= 0 or the square shares no pixel with the
 * frame (zeros written; parity unpinned: the reference raises or, through numpy's negative-slice
 * wrap-around, returns a black crop, depending on the side the square lies on).  (ABI 9 addition) */
int spe_preprocess_submission(void* stream, const uint8_t* frames, int batch, int height, int width, int channels,
                              const double* bbox_xxyy, int size, float* images, uint8_t* crops_u8, float* clip_bbox,
                              int32_t* status);

/* Baseline-JPEG decode of grayscale frames on the device: the decode half of
 * `Image.open(img_path).convert('RGB')` in SpeedTrain.__getitem__ (REV/datasets/speed.py:209-210;
 * Pillow / libjpeg-turbo, islow IDCT), which the reference runs in DataLoader worker processes
 * (REV/main.py:252-254).  data: device bytes holding the batch's JPEG files; offsets / sizes:
 * device int64 [B] (file b = data[offsets[b] .. offsets[b] + sizes[b])); every file must be a
 * height x width 8-bit single-component sequential Huffman JPEG (SOF0/SOF1, restart intervals
 * allowed) of at most max_bytes_per_image bytes.  frames: device uint8 [B,height,width], the
 * 1-channel input spe_preprocess takes.  status (nullable): [B] 0 ok, 1 unsupported coding
 * (progressive, arithmetic, 12-bit, colour), 2 corrupt stream, 3 frame size != height x width,
 * 4 stream exceeds the workspace plan; a non-zero image gets a zero frame.  workspace: device
 * bytes, spe_jpeg_workspace_bytes(batch, height, width, max_bytes_per_image) of them. */
int64_t spe_jpeg_workspace_bytes(int batch, int height, int width, int64_t max_bytes_per_image);
int spe_jpeg_decode(void* stream, const uint8_t* data, const int64_t* offsets, const int64_t* sizes, int batch,
                    int height, int width, int64_t max_bytes_per_image, uint8_t* frames, int32_t* status,
                    void* workspace, int64_t workspace_bytes);

/* SetCriterion.forward with its HungarianMatcher (REV/models/detr_speed.py:214-261,
 * REV/models/matcher.py:60-88) for `layers` decoder layers (aux first, last layer last), the
 * logging half of evaluate() (REV/engine.py:99-112).  Device pointers: logits [L,B,Q,C] (C = 12 in
 * the reference; class C-1 is no-object), points [L,B,Q,2], tgt_labels int32 [B,T] (a label outside
 * [0,C) counts as class C-1, as in spe_criterion_sigma), tgt_points [B,T,2] (crop-normalised), match
 * int32 [L,B,T] (query matched to each target), losses fp64 [L,4] = loss_ce, class_error,
 * cardinality_error, loss_points.  num_points: targets per rank averaged over ranks, >= 1
 * (REV/models/detr_speed.py:235-244), the divisor of loss_points alone.  1 <= Q <= 64,
 * 1 <= T <= min(Q, 32), 2 <= C <= 32, num_points > 0, else SPE_E_ARG before any launch. */
int spe_criterion(void* stream, const float* logits, const float* points, const int32_t* tgt_labels,
                  const float* tgt_points, int layers, int batch, int num_queries, int num_classes, int num_targets,
                  float cost_class, float cost_pts, float eos_coef, double num_points, int32_t* match, double* losses);

/* The UNC RT-DETR SetCriterion.forward with its HungarianMatcher (UNC/src/zoo/rtdetr/
 * rtdetr_criterion.py:280-337, matcher.py:53-117) for `layers` outputs (the main output first,
 * then aux_outputs in order), the logging half of UNC/solver/speed_engine.py:145-173.  Device
 * pointers: logits [L,B,Q,C], points [L,B,Q,2], log_sigmas [L,B,Q,2] (pred_sigmas),
 * layer_has_sigma int32 [L] (0: the layer has no sigma and scores with s = 0, like the encoder
 * top-k entry; log_sigmas may be NULL when every flag is 0), tgt_labels int32 [B,T] (a label
 * outside [0,C) counts as class C-1), tgt_points [B,T,2] (crop-normalised), match int32 [L,B,T]
 * (query matched to each target), losses fp64 [L,6] = loss_ce, class_error, cardinality_error,
 * loss_bbox (points: sum |p - t| / num_boxes), loss_bbox (points_uncert: sum (|p - t| exp(-s) +
 * 0.5 s) / num_boxes), points_different (sum (p - t)), all unweighted.  Matching cost
 * cost_bbox * L1 - cost_class * prob[label] with prob = sigmoid(logit) when sigmoid_cost (the
 * speed configs' use_focal_loss), else softmax.  num_boxes: the plain target count (> 0).
 * Q <= 64, T <= min(Q, 32), C <= 64, else SPE_E_ARG before any launch.  Like spe_criterion it
 * neither allocates nor synchronises once its per-stream scratch has the batch's size. */
int spe_criterion_sigma(void* stream, const float* logits, const float* points, const float* log_sigmas,
                        const int32_t* layer_has_sigma, const int32_t* tgt_labels, const float* tgt_points,
                        int layers, int batch, int num_queries, int num_classes, int num_targets,
                        float cost_class, float cost_bbox, int sigmoid_cost, float eos_coef, double num_boxes,
                        int32_t* match, double* losses);

/* Multi-checkpoint ensemble front end (Multi_Mean_PoseSolver, REV/utils/speed_eval.py:42-100;
 * REV/gen_submission_multi.py:145-186): fuses M models' PostProcess outputs per image -- labels
 * in first-seen order, per label the mean of its points after the 3-sigma filter -- into
 * fused_points [B,C-1,2] + one-hot fused_probs [B,C-1,C], the input spe_pnp_batch then solves
 * (RANSAC_P3P_LM, like the reference).  points [M,B,Q,2] px, probs [M,B,Q,C]; M * Q <= 256 and
 * 2 <= C <= 17, else SPE_E_ARG before any launch.  A label may pool all M * Q points: the fp64 sums of
 * the filter's standard deviation follow numpy's pairwise summation over that whole range (one block
 * up to 128 values, split in two above), so the fused points equal numpy's bit for bit. */
int spe_ensemble_fuse(void* stream, const float* points_px, const float* probs, int models, int batch,
                      int num_queries, int num_classes, float* fused_points, float* fused_probs);

/* Sigma-weighted multi-checkpoint ensemble: fuses M sigma models' PostProcess outputs per image into one
 * keypoint set WITH a sigma, so that an ensemble can feed the sigma-weighted solvers, spe_self_assess and
 * spe_pose_covariance.  No reference code exists (UNC/utils/speed_eval_ceres.py:405-462 is the unweighted
 * mean of spe_ensemble_fuse); this comment is the definition (parity unpinned).  All pointers are device
 * memory: points_px [M,B,Q,2], probs [M,B,Q,C], sigmas [M,B,Q,2] fp32 (sigmas in the model's unit);
 * sigma_scale [B,2] (nullable: scale 1) is the number of pixels per sigma unit and axis, the crop's width
 * and height as spe_pose_covariance takes it.  K = C - 1 landmarks.
 *
 * Measurements.  A query's label is the argmax of its probability row (the lower class on ties) and its
 * score that maximum; background (label K) is dropped.  Per model and label the measurement is the
 * label's highest-score query (the earlier query on ties): spe_pnp_batch's selection, so a model gives at
 * most one measurement per label and the measurements of a label are independent (unlike the REV rule,
 * which pools every foreground query).  With x, y the query's point and u = sigma * scale per axis (the
 * product taken in fp64), the measurement is usable when the image's two scales are finite and positive
 * and x, y, ux, uy and the score are all finite; its effective sigma is s = max(u, sigma_floor) per axis.
 * n_pooled counts a label's measurements, usable or not.  A label without a usable one is not emitted.
 *
 * Fusion, per emitted label, in fp64, every sum taken one term after the other in ascending model order
 * and without contraction.  Over the kept measurements (at first the usable ones), per axis:
 *     w_i = 1 / (s_i * s_i),   mu = (sum w_i * x_i) / (sum w_i)
 * Gate: while 3 or more are kept, d_i^2 = dx * dx + dy * dy with dx = (x_i - mu_x) / s_ix and dy alike;
 * if sqrt of the largest d_i^2 (the lowest model on ties) exceeds `gate`, that measurement is dropped, mu
 * is recomputed over the rest and the test repeats.  Two measurements are never gated.  n_kept counts
 * what is left.  Fused sigma per axis:
 *     sqrt(1 / sum w_i) * f / scale,   f = max(1, sqrt(chi2 / (n_kept - 1))),   chi2 = sum w_i * (e_i * e_i),
 * e_i = x_i - mu; f = 1 when n_kept = 1.  f is the Birge ratio: scatter beyond what the sigmas predict
 * widens the result.  The division by the scale returns the sigma in the input's unit, so downstream
 * calls pass clip_bbox exactly as for one model.  Fused score = (sum score_i) / n_kept.
 *
 * Outputs.  Row r of an image is its r-th emitted label in first-seen order (spe_ensemble_fuse's order:
 * model-major, then by query, over all foreground queries of the emitted labels), the layout
 * spe_pnp_batch, spe_self_assess and spe_pose_covariance read.  fused_points [B,K,2]; fused_probs
 * [B,K,C]: the fused score in the label's column and 0 elsewhere (the row need not sum to 1; its argmax
 * is the label for a positive score); fused_sigmas [B,K,2]; n_pooled, n_kept [B,K].  Each fp32 output is
 * the fp64 value rounded once.  The rows after the last emitted label are unused: probability 1 at
 * background and 0 in every other output.  No NaN leaves the kernel.
 *
 * 1 <= M <= 16, M * Q <= 256, 2 <= C <= 17, B >= 1, every pointer but sigma_scale non-NULL, gate > 0,
 * sigma_floor positive and finite, else SPE_E_ARG before any launch with the outputs untouched.  One
 * launch; no allocation, no scratch, no synchronisation. */
int spe_ensemble_fuse_sigma(void* stream, const float* points_px, const float* probs, const float* sigmas,
                            const float* sigma_scale, int models, int batch, int num_queries, int num_classes,
                            float sigma_floor, float gate, float* fused_points, float* fused_probs,
                            float* fused_sigmas, int32_t* n_pooled, int32_t* n_kept);

/* Lens distortion in front of the solvers.  The reference hands Camera.dist to cv2.solvePnPRansac,
 * cv2.solvePnPGeneric and cv2.undistortPoints (UNC/utils/speed_eval.py, speed_eval_ceres.py,
 * val_p_which_p.py); the solver entries above take K alone.  spe_undistort_points turns distorted pixel
 * points into ideal pixel points K . undistort(K^-1 p) and maps the per-axis sigma alongside, so every
 * solver entry, spe_self_assess, spe_pose_covariance and the ensemble fusions then run unchanged on a
 * pinhole problem.  All pointers are device memory; points and sigmas [B,Q,2] fp32, 8-byte aligned;
 * K 3x3 row-major fp64 (fx = K[0], fy = K[4], cx = K[2], cy = K[5]); dist = (k1, k2, p1, p2, k3) fp64,
 * OpenCV's five-coefficient model.  Everything is computed in fp64, each step rounded on its own.
 *
 * Distort, of an ideal normalised point x, y with r2 = x * x + y * y:
 *     rad = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
 *     xd  = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
 *     yd  = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
 *     ud  = fx * xd + cx,  vd = fy * yd + cy
 * Undistort: cv2.undistortPoints' fixed-point iteration, run for exactly `iters` rounds with no early
 * exit on a tolerance (5 = cv2's TermCriteria(MAX_ITER, 5, ...)).  x0 = (u - cx) / fx, y0 = (v - cy) / fy,
 * x, y start at x0, y0, and each round computes
 *     icd = 1 / rad(x, y),  dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x),  dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
 *     x = (x0 - dx) * icd,  y = (y0 - dy) * icd
 * The ideal point is (fx * x + cx, fy * y + cy), rounded once to fp32.
 *
 * Sigma.  sigmas is in the caller's unit and sigma_scale [B,2] (nullable: 1) the pixels per unit and
 * axis, as spe_pose_covariance takes them.  D = d(ud, vd) / d(ui, vi) is the distort map's Jacobian in
 * pixels, in closed form at the undistorted point (g = d rad / d r2 = (3 * k3 * r2 + 2 * k2) * r2 + k1,
 * c = 2 * x * y * g + 2 * p1 * x + 2 * p2 * y):
 *     D11 = rad + 2 * x * x * g + 2 * p1 * y + 6 * p2 * x      D12 = c * (fx / fy)
 *     D21 = c * (fy / fx)                                      D22 = rad + 2 * y * y * g + 6 * p1 * y + 2 * p2 * x
 * and A = D^-1.  With ux = sigma_x * sx, uy = sigma_y * sy:
 *     sigma_x' = sqrt(A11^2 * ux^2 + A12^2 * uy^2) / sx,   sigma_y' = sqrt(A21^2 * ux^2 + A22^2 * uy^2) / sy
 * The cross term of A Sigma A^T is dropped: the solvers and the covariance take one sigma per axis.  A
 * scale that is not positive and finite gives a sigma that is not finite, which spe_pose_covariance
 * reports as its status 3.
 *
 * status [B,Q] (nullable): 0, or 1 where icd is not positive and finite in some round (cv2's icdist < 0
 * bail-out) or |det D| is not positive and finite; such a point and its sigma are returned as they came.
 * When all five coefficients are exactly zero the points and sigmas are copied bit for bit.  sigmas,
 * sigma_scale, sigmas_ideal and status are nullable; sigmas_ideal without sigmas, batch < 1,
 * num_queries < 1, batch * num_queries > 2^30, iters outside [1, 64] or a misaligned array is SPE_E_ARG
 * before any launch.  points_ideal may be points_px and sigmas_ideal may be sigmas (in place).  One launch,
 * one thread per point; no allocation, no scratch, no synchronisation.
 *
 * PARITY UNPINNED: cv2 is absent here; tests/lens_ref.py restates this comment in numpy.  One place
 * differs from cv2 by design.  cv2 undistorts before it minimises (EPnP, P3P, the ITERATIVE LM, the
 * reference's ceres_pnp all work on undistortPoints' output), so the minimisers see what they see here.
 * But cv2's RANSAC inlier test (projectPoints with distCoeffs against the observed points) and the
 * reference's epnp_init error measure distance in the distorted image, and the solvers here measure it
 * between ideal points.  The two differ by the local stretch of the lens: max |D - I| = 0.043 over a
 * 1920 x 1200 frame (0.047 with a 200 px margin) for k1 = -0.224, k2 = 0.514, p1 = -6.6e-4, p2 = -2.1e-4,
 * k3 = -0.131 at the SPEED K, so only a residual within about 4 % of the threshold is classified
 * differently. */
int spe_undistort_points(void* stream, const float* points_px, const float* sigmas, const float* sigma_scale,
                         int batch, int num_queries, const double* K, const double* dist, int iters,
                         float* points_ideal, float* sigmas_ideal, uint8_t* status);
/* The distort map above on ideal pixel points [B,Q,2] -> distorted pixel points (fp32, rounded once);
 * points_px may be points_ideal.  The same argument checks. */
int spe_distort_points(void* stream, const float* points_ideal, int batch, int num_queries, const double* K,
                       const double* dist, float* points_px);

/* PostProcess alone (REV/models/detr_speed.py:266-293). */
int spe_postprocess(void* stream, const float* logits, const float* points, const float* clip_bbox, int batch,
                    int num_queries, float* probs, float* points_px);

/* Batched solver (SimplePoseSolver.__call__ per image, REV/utils/speed_eval.py:164-242;
 * SimplePoseSolverSigma, UNC/utils/speed_eval.py:332-420).  All pointers are device memory.
 * K: 3x3 row-major fp64; world: [C-1][3] fp64 landmarks (REV/all_result.json).
 * quat: [B,4] (float32 values, Blender order w,x,y,z); tvec/rvec: [B,3] fp64;
 * corr_label: [B,16] label of each correspondence in first-seen order (-1 padded);
 * inlier_mask: [B] bit i = correspondence i is an inlier; 0 where the RANSAC modes end without a pose,
 * the direct solve on exactly 4 (P3P) or 5 (EPnP) points included.  repro_per_image: [B] fp32 thresholds that
 * replace `repro` image by image (EPnPCeresSolver.get_repro_th of each image's box area).  Nullable:
 * sigmas, rvec, status, n_corr, corr_label, inlier_mask, repro_per_image. */
int spe_pnp_batch(void* stream, const float* points_px, const float* probs, const float* sigmas, int batch,
                  int num_queries, int num_classes, const double* K, const double* world, int mode, float repro,
                  int ransac_iters, double confidence, float* quat, double* tvec, double* rvec, int32_t* status,
                  int32_t* n_corr, int32_t* corr_label, uint32_t* inlier_mask, const float* repro_per_image);

/* SPE_PNP_EXHAUSTIVE (see the solver modes): spe_pnp_batch's arguments without the RANSAC ones, plus
 * topk in [1,64]; cand_index [B]: the winning hypothesis's subset index (its rank in
 * itertools.combinations(range(n_corr), 4)), -1 without a pose; repro_final [B]: the image's threshold
 * after growth.  inlier_mask is the winner's inlier set at the threshold it was tested with.  Both new
 * outputs are nullable.  num_classes - 1 <= 16.  Hypothesis records live in per-(device, stream)
 * scratch like the sigma mode's: no allocation or synchronisation once it has its size. */
int spe_pnp_exhaustive(void* stream, const float* points_px, const float* probs, const float* sigmas, int batch,
                       int num_queries, int num_classes, const double* K, const double* world, float repro, int topk,
                       float* quat, double* tvec, double* rvec, int32_t* status, int32_t* n_corr,
                       int32_t* corr_label, uint32_t* inlier_mask, const float* repro_per_image,
                       int32_t* cand_index, float* repro_final);
/* The same with a stage mask (measurement only): 1 = the hypothesis kernel, 2 = selection + refinement on
 * the records a stage-1 call left in this stream's scratch, 3 = both. */
int spe_debug_pnp_exhaustive_stages(void* stream, const float* points_px, const float* probs, const float* sigmas,
                                    int batch, int num_queries, int num_classes, const double* K, const double* world,
                                    float repro, int topk, float* quat, double* tvec, double* rvec, int32_t* status,
                                    int32_t* n_corr, int32_t* corr_label, uint32_t* inlier_mask,
                                    const float* repro_per_image, int32_t* cand_index, float* repro_final, int stages);

/* Self-assessment filter over the sigma solver's output (BASELINE config 4).  No reference code
 * exists: the UNC README (ROOT/README.md:15-20) names the mechanism and the commented gate
 * `s_ > 0.5 and sig.mean() < 5` (UNC/utils/speed_eval_ceres.py:110-114) is its only trace, so
 * the rule is defined here (parity unpinned): over the RANSAC inliers of each image,
 * mean_sigma = mean sigma (both axes); n_confident = #inliers with score > score_th and mean
 * sigma < sigma_th; reliable = pose solved (status 0 or 3) and n_confident >= min_inliers and
 * mean_sigma < sigma_th.  Inputs are spe_forward's probs/sigmas and spe_pnp_batch's status /
 * corr_label / inlier_mask; all device pointers. */
int spe_self_assess(void* stream, const float* probs, const float* sigmas, const int32_t* status,
                    const int32_t* corr_label, const uint32_t* inlier_mask, int batch, int num_queries,
                    int num_classes, float score_th, float sigma_th, int min_inliers, float* mean_sigma,
                    int32_t* n_confident, uint8_t* reliable);

/* Pose covariance from the keypoint sigmas: the first-order (Gauss-Newton) covariance of the solved
 * pose under independent Gaussian keypoint noise with the predicted sigmas.  No reference code exists;
 * this comment is the definition.  Inputs are spe_forward's probs / sigmas and a solver's status /
 * corr_label / inlier_mask / rvec / tvec (spe_pnp_batch in any mode, spe_pnp_exhaustive); all device
 * pointers; K and world as for spe_pnp_batch (world is read as fp64, as passed).
 *
 * Correspondences.  Correspondence i of image b has label corr_label[b][i]; its query is the one the
 * solver selected for that label (highest foreground score, the first on ties: the selection
 * spe_self_assess re-derives, the same code).  Only correspondences whose bit is set in inlier_mask
 * take part, and only where the label is a landmark (0 <= label < num_classes - 1) that some query
 * carries; the inlier count below counts those.
 *
 * Sigma.  sigmas [B,Q,2] is PostProcess's sigma, exp(pred_sigmas), in the caller's unit; sigma_scale
 * [B,2] (nullable: sigma is in pixels already) multiplies it per image and axis into pixels, the product
 * taken in fp64.  Effective sigma = max(sigma * scale, sigma_floor); sigma_floor must be positive and finite.
 * A product that is not finite on either axis of a taking-part correspondence is a bad sigma.
 *
 * Perturbation.  R <- exp([dw]x) R, t <- t + dt in the camera frame; state order (dw, dt), rad then
 * metres.  Per taking-part correspondence with landmark X: Xc = R X + t = (x, y, z) and
 *     J = [[fx/z, 0, -fx x/z^2], [0, fy/z, -fy y/z^2]] . [ -[R X]x | I ]      (2x6, fp64; fx = K[0], fy = K[4])
 * Information H = sum J^T diag(1/sx^2, 1/sy^2) J over the correspondences in fp64, by a fixed summation
 * tree (correspondence i with i^8, then ^4, ^2, ^1; absent ones contribute 0), so two runs give the same
 * bits.  Covariance = H^-1 by Cholesky of the Jacobi-scaled D^-1/2 H D^-1/2, D = diag H (the rad and
 * metre blocks differ by about z^2), unscaled afterwards.
 *
 * Outputs: cov [B,6,6] fp64, symmetric, fully written; sigma_rot [B] = sqrt(tr cov_ww) rad; sigma_t [B,3]
 * = sqrt of the translation diagonal, metres; pred_score [B] = sigma_rot + sqrt(tr cov_tt) / |t|, the
 * first-order RMS prediction of the SPEED score (angle error + relative translation error); cov_status [B]:
 *     0 ok
 *     1 no pose (solver status not 0 or 3)
 *     2 fewer than 3 taking-part inliers
 *     3 bad sigma
 *     4 singular: a taking-part point with z <= 0 (or not a number), a diagonal of H that is not positive
 *       and finite, a pivot of the scaled matrix <= 64 * DBL_EPSILON, or a result that is not finite (|t| = 0)
 * tested in this order, the first that applies.  For a non-zero status every numeric output of the image is
 * 0: no NaN leaves the kernel.  num_queries <= 64, 2 <= num_classes <= 17, batch >= 1, else SPE_E_ARG
 * before any launch.  One launch; no allocation, no scratch, no synchronisation. */
int spe_pose_covariance(void* stream, const float* probs, const float* sigmas,
                        const float* sigma_scale, const int32_t* status,
                        const int32_t* corr_label, const uint32_t* inlier_mask,
                        const double* rvec, const double* tvec, int batch,
                        int num_queries, int num_classes, const double* K,
                        const double* world, float sigma_floor, double* cov,
                        float* sigma_rot, double* sigma_t, float* pred_score,
                        int32_t* cov_status);

/* Calibration records: what a predicted sigma, covariance and score are compared with when the ground
 * truth pose is known.  No reference code exists (the reference's self-assessment is commented out); this
 * comment is the definition, all of it in fp64.  Inputs are those of spe_pose_covariance (device pointers,
 * the same K and world, corr_label [B,16]) plus points_px [B,Q,2] in the image the pose was solved in, the
 * ground truth q_gt [B,4] / t_gt [B,3], and spe_pose_covariance's cov [B,6,6] / cov_status [B].
 *
 * sigma_gain (finite and > 0, else SPE_E_ARG) is the calibration factor under test: it multiplies the
 * sigma before the floor, effective sigma = max(sigma * scale * gain, sigma_floor), and the covariance is
 * read as cov * gain^2.  cov is therefore the covariance at gain 1.
 *
 * Ground-truth rotation.  R_gt is the rotation whose quaternion (w, x, y, z), as spe_pnp_batch emits it
 * (Blender's mat3_to_quat of the camera-from-body R), is q_gt / |q_gt|:
 *     R_gt = [[1-2(yy+zz), 2(xy-zw), 2(xz+yw)], [2(xy+zw), 1-2(xx+zz), 2(yz-xw)], [2(xz-yw), 2(yz+xw), 1-2(xx+yy)]]
 * so a pose whose emitted quaternion equals q_gt has no rotation error; spe_speed_score pairs the two
 * quaternions component by component, the same convention.
 *
 * Pose error, in spe_pose_covariance's perturbation convention R_pr = exp([dw]x) R_gt, t_pr = t_gt + dt:
 * with q_pr = (cos(|r|/2), sin(|r|/2) r/|r|) of rvec and q_rel = q_pr (x) conj(q_gt / |q_gt|) = (w, v), sign
 * chosen so that w >= 0,  dw = 2 atan2(|v|, w) v/|v|  (0 where |v| = 0; never acos, so that a small angle
 * keeps its digits) and dt = tvec - t_gt.  delta [B,6] = (dw, dt).  |dw| is spe_speed_score's s_q of the pair.
 *
 * NEES.  nees [B,3] = (delta^T S^-1 delta, dw^T S_ww^-1 dw, dt^T S_tt^-1 dt) with S = cov * gain^2 and its two
 * marginal 3x3 blocks: 6, 3 and 3 degrees of freedom.  Each is one Cholesky solve of the Jacobi-scaled
 * matrix D^-1/2 S D^-1/2, D = diag S; no inverse is formed.
 *
 * Keypoint z-scores.  For landmark l (0 <= l < L = num_classes - 1) the query is the one the solver's
 * selection gives the label (highest score, the first on ties; the same code as spe_self_assess and
 * spe_pose_covariance).  z [B,L,2] = (p_sel - pi(R_gt X_l + t_gt)) / effective sigma, per axis, with pi the
 * pinhole projection (fx x/z + cx, fy y/z + cy).  kp_flags [B,L]: bit 0 valid -- some query carries the
 * label, the ground-truth point has z > 0, and the point, the sigma * scale * gain product and the z-score are
 * finite; bit 1 taking-part inlier -- the solver has a pose (status 0 or 3), a correspondence with this
 * label has its bit set in inlier_mask, and some query carries the label (spe_pose_covariance's rule).  The
 * bits are independent; where bit 0 is clear z = 0.
 *
 * calib_status [B], the first that applies:
 *     0 ok
 *     1 ground truth unusable: |q_gt| zero or not finite, or t_gt not finite
 *     2 no pose (solver status not 0 or 3)
 *     3 no covariance (cov_status != 0)
 *     4 singular: delta not finite, a diagonal of S not positive and finite, a pivot of a scaled matrix
 *       <= 64 * DBL_EPSILON, or a NEES that is not finite
 * delta is written for status 0, 3 and 4 (all zero where it is not finite), nees for status 0, z and
 * kp_flags for every status but 1; everything else is 0, and no NaN leaves the kernel.  num_queries <= 64,
 * 2 <= num_classes <= 17, batch >= 1, sigma_floor positive and finite, else SPE_E_ARG before any launch.
 * One launch (one wave per image); no allocation, no scratch, no synchronisation. */
int spe_calibration_records(void* stream, const float* points_px, const float* probs, const float* sigmas,
                            const float* sigma_scale, float sigma_floor, const int32_t* status,
                            const int32_t* corr_label, const uint32_t* inlier_mask, const double* rvec,
                            const double* tvec, const double* q_gt, const double* t_gt, const double* cov,
                            const int32_t* cov_status, int batch, int num_queries, int num_classes,
                            const double* K, const double* world, double sigma_gain, double* delta, double* nees,
                            double* z, uint8_t* kp_flags, int32_t* calib_status);

/* Landmark reconstruction: the body-frame 3-D landmarks (the `world` table every entry above reads) from 2-D
 * keypoint observations in views of known pose.  The paper obtains its table by multi-view triangulation;
 * that code is not in the reference (it ships the result, all_result.json 'pt'), so this comment is the
 * definition, all of it in fp64, every step rounded on its own.  All pointers are device memory.
 *
 * Observations.  N = num_views, L = num_landmarks (1 <= L <= 16).  obs_px [N,L,2] pixels; obs_sigma [N,L,2]
 * pixels (nullable: every sigma is 1 px); obs_valid [N,L] u8 (0: no observation); q_gt [N,4] / t_gt [N,3] the
 * view's pose, R_gt by spe_calibration_records' formula (camera-from-body, X_cam = R_gt X + t_gt); K 3x3
 * row-major, read as fx = K[0], fy = K[4], cx = K[2], cy = K[5] (no skew).  An observation is skipped -- it
 * enters no sum and no NaN propagates -- where obs_valid is 0, the view's |q_gt| is zero or not finite, t_gt
 * is not finite, the point is not finite, or sigma * sigma_gain is not finite on either axis.  Effective sigma
 * = max(sigma * sigma_gain, sigma_floor) per axis, spe_calibration_records' rule.
 *
 * Stage 0, the linear start (skipped when world_init [L,3] is given: that is the start point).  With
 * u = (px - cx) / fx, v = (py - cy) / fy and r1, r2, r3 the rows of R_gt, a view gives the two rows
 *     (r1 - u r3) . X = -(t1 - u t3)        weight (fx / sigma_x)^2
 *     (r2 - v r3) . X = -(t2 - v t3)        weight (fy / sigma_y)^2
 * summed over the landmark's views into the 3x3 normal matrix A = sum w a a^T and the vector sum w a b, solved
 * by Cholesky of the Jacobi-scaled D^-1/2 A D^-1/2, D = diag A (chol3_factor / chol3_backsolve of pnp_math.h).
 *
 * Stage 1, the refinement: `iterations` Levenberg-Marquardt steps on r = ((px - pi_x) / sigma_x, (py - pi_y)
 * / sigma_y), pi = (fx x/z + cx, fy y/z + cy) of (x, y, z) = R_gt X + t_gt.  An evaluation at a point X runs
 * over the landmark's views that are not skipped and have z > z_min (and a finite |r|): the used views.  With
 * h = huber and |r| the norm of the view's two components, in sigma units: weight w = 1 and rho = |r|^2, or,
 * where h > 0 and |r| > h, w = h / |r| and rho = 2 h |r| - h^2.  J = d pi / d X over sigma, per axis (2x3):
 *     Jx = (fx / z / sigma_x) (r1 - (x/z) r3),   Jy = (fy / z / sigma_y) (r2 - (y/z) r3)
 * H = sum w J^T J, g = sum w J^T r, robust cost = sum rho, n = the number of used views, and sum of
 * (px - pi_x)^2 + (py - pi_y)^2.  The start point is evaluated first: fewer than 2 used views there is status
 * 1, otherwise it is the accepted point and lambda = 1e-3.  A step solves (H + lambda diag H) d = g at the
 * accepted point (Cholesky of D^-1/2 H D^-1/2 + lambda I) and evaluates the candidate X + d: it is accepted,
 * with lambda / 10, when its robust cost is lower and it uses no fewer views than the accepted point;
 * otherwise the accepted point, its H and g are kept, with lambda * 10.  The step count is fixed; nothing is
 * read back between steps.
 *
 * Summation.  Every sum over views is taken in one fixed order: view n is lane n % 64 of wave n / 64; a wave's
 * lanes are joined by the xor butterfly 32, 16, 8, 4, 2, 1 (skipped and absent views contribute 0); the wave
 * partials w, w + 64, w + 128, .. are added in that order by lane w % 64 of a second wave and joined by the
 * same butterfly.  No atomics: two runs give the same bits.
 *
 * Outputs, at the accepted point: world [L,3]; cov [L,3,3] = H^-1 (Cholesky of the Jacobi-scaled H, unscaled
 * afterwards, symmetric, fully written; not multiplied by chi2); chi2 [L] = the robust cost; n_used [L] i32;
 * rms_px [L] = sqrt(sum((px - pi_x)^2 + (py - pi_y)^2) / n), unweighted; obs_flags [N,L] u8: bit 0 the
 * observation is used at the final point, bit 1 it is beyond the Huber threshold there (h > 0 and |r| > h;
 * only with bit 0).  lm_status [L], the first that applies:
 *     0 ok
 *     1 fewer than 2 usable views (stage 0: not skipped; the start point's evaluation: used)
 *     2 degenerate: a diagonal of a matrix to factor that is not positive and finite, or a pivot of the
 *       scaled matrix <= 64 * DBL_EPSILON (rays parallel, identical poses)
 *     3 a start point, candidate or result that is not finite
 * For a non-zero status the landmark's world, cov, chi2, n_used and rms_px are 0, its obs_flags are 0, and it
 * takes no part in later launches: no NaN leaves the kernels.
 *
 * spe_landmarks_solve launches stage 0 (2 launches), iterations + 1 evaluate / update pairs and the flags
 * kernel on `stream`; no allocation, no synchronisation; it works in `scratch`, caller-owned device memory,
 * 8-byte aligned, of at least spe_landmarks_scratch_bytes(num_views, num_landmarks) bytes (0 for arguments
 * out of range), whose contents mean nothing between calls.  SPE_E_ARG before any launch: a null required
 * pointer, num_views < 1, num_landmarks outside [1, 16], iterations outside [0, 64], sigma_floor or sigma_gain
 * not positive and finite; SPE_E_WORKSPACE: a scratch misaligned or too small.  huber <= 0 switches the
 * robust weight off.
 *
 * spe_landmark_observations turns model output into the observation layout, one launch, one wave per image:
 * for landmark l (0 <= l < L = num_classes - 1) the query is the one the solver's selection gives the label
 * (highest score, the first on ties; the same code as spe_pnp_batch and spe_calibration_records).  Image b is
 * written at row row_offset + b of obs_px / obs_sigma / obs_valid [rows,L,.]: obs_px = the query's point;
 * obs_sigma (nullable) = sigmas * sigma_scale, the fp64 product, sigmas [B,Q,2] and sigma_scale [B,2] as
 * spe_pose_covariance takes them (sigmas null: 1; sigma_scale null: the sigmas are pixels); obs_valid = 1.
 * A label no query carries gives point 0, sigma 1, obs_valid 0.  num_queries <= 64, 2 <= num_classes <= 17,
 * batch >= 1, row_offset >= 0, else SPE_E_ARG before any launch. */
int spe_landmark_observations(void* stream, const float* points_px, const float* probs, const float* sigmas,
                              const float* sigma_scale, int batch, int num_queries, int num_classes,
                              int64_t row_offset, double* obs_px, double* obs_sigma, uint8_t* obs_valid);
int64_t spe_landmarks_scratch_bytes(int num_views, int num_landmarks);
int spe_landmarks_solve(void* stream, const double* obs_px, const double* obs_sigma, const uint8_t* obs_valid,
                        const double* q_gt, const double* t_gt, int num_views, int num_landmarks, const double* K,
                        const double* world_init, int iterations, double huber, double sigma_floor,
                        double sigma_gain, double z_min, void* scratch, int64_t scratch_bytes, double* world,
                        double* cov, double* chi2, int32_t* n_used, double* rms_px, uint8_t* obs_flags,
                        int32_t* lm_status);

/* speed_score per image (REV/utils/speed_eval.py:245-262), device pointers. */
int spe_speed_score(void* stream, const float* quat, const double* tvec, const double* q_gt, const double* t_gt,
                    int batch, double* s_t, double* s_q);

/* Per-launch profiling of spe_forward with HIP events on the launch stream (no reference
 * counterpart; used by bench.py for the roofline).  begin: every later launch whose kind starts
 * with `kind_prefix` ("" = all; kinds: conv.*, gemm.*, attn.enc, attn.dec_*, ln.*, eltwise.*,
 * heads) is bracketed by events.  end: stops recording, waits for the events, returns the
 * record count.  get: record i -> kind, elapsed ms, algorithmic flops and bytes. */
int spe_model_profile_begin(spe_model* m, const char* kind_prefix);
int spe_model_profile_end(spe_model* m);
int spe_model_profile_get(const spe_model* m, int i, char* kind, int kind_len, double* ms, double* flops,
                          double* bytes);

/* Kernel test hooks: launch one kernel family on caller buffers (tests/test_gpu_kernels.py).
 * gemm: C[M,N] = act(A . W^T + bias + R) with act = act_code & 255 (0 none, 1 ReLU, 2 SiLU, 3
 * exact GELU); bit 8 of act_code adds R after the activation instead; mode 0 linear (A[m*lda+k]), 1 linear + P[(m%prow)
 * *ldp+k] added to A, 2 implicit-GEMM conv over NHWC A [*,H,W,Cin]; W is [N][ldb] (ldb % 64 == 0);
 * vt_T > 0 stores head-transposed C[((n/256)*vt_B + m/vt_T)*256 + n%256][m%vt_T]; r_period > 0
 * reads the residual row-periodically, R[(m % r_period)*ldr + n].  bf16 problems that fill the chip
 * with 256-row tiles run the direct-to-LDS kernel (gemm2.hip), the rest the 128x128 kernel.
 * attention: per (b,h) softmax(scale Q K^T) V with Q/K rows b*T+i at column h*32, V^T [B][H][32][Tk].
 * Bit 9 of the gemm act_code and bit 8 of the attention dtype select the swizzled V^T layout the
 * encoder uses with 16-bit operands (token t of every 16-token group stored at position t with
 * bits 2 and 3 swapped; Tk % 16 == 0): the v projection writes it, the LDS-DMA attention reads it. */
int spe_debug_gemm(void* stream, int dtype, int mode, const void* A, int lda, const void* P, int ldp, int prow, int H,
                   int W, int Cin, int KH, int KW, int stride, int pad, const void* Bw, int ldb, int M, int N, int K,
                   const float* bias, const void* R, int ldr, int act_code, void* C, int ldc, int out_f32, int vt_T,
                   int vt_B, int r_period, const float* ln_g, const float* ln_b, int out_f16);
/* (out_f16: bf16 launches store fp16 instead of bf16.  ln_g/ln_b non-null: post-norm LayerNorm over each output row fused into the epilogue; bf16,
 * N == 256 and enough rows for the large-tile kernel, else SPE_E_LAUNCH) */
/* kernel family that served this thread's last gemm launch: 0 the 128x128 kernel, 1 the large-tile
 * kernels (gemm2.hip), 2 the persistent streaming kernel for short-K problems (gemm_stream.hip),
 * 3 the patch-staged 3x3 conv (pconv.hip), 4 the projection + residual + LayerNorm (lnproj.hip),
 * 5 the fp32x6 three-way split kernel (gemm.hip), 6 its LDS-DMA form (gemm.hip gemm_x6d), 7 the fp32h3
 * scaled fp16 split kernel (gemm.hip gemm_h3d), 8 its persistent row-store form (gemm.hip gemm_h3p) */
int spe_debug_gemm_path(void);
/* fp32h3 (gemm.hip gemm_h3d): C = act((A . W^T) + bias + R) on fp32 A (LINEAR or CONV geometry as
 * spe_debug_gemm) with the weights given as the finalize form -- planes = fp16 [2][plane_rows][ldb]
 * holding hi, lo of W[n] * 2^e_n, sinv[n] = 2^-e_n -- and amax_a = device max |A| (nullable: scale
 * 1).  amax_c (nullable): max |stored C| * (amax_c_mul or 1) atomically maxed into it (float bits).
 * (Round 5 removed its LayerNorm-epilogue form: the model runs the persistent GEMM + the LayerNorm
 * kernel, measured faster.) */
int spe_debug_gemm_h3(void* stream, int mode, const void* A, int lda, int H, int W, int Cin, int KH, int KW, int stride,
                      int pad, int ldb, int M, int N, int K, const float* bias, const void* R, int ldr, int act_code,
                      void* C, int ldc, const void* planes, int plane_rows, const float* sinv, const float* amax_a,
                      float* amax_c, float amax_c_mul);
/* fp32h3 one-pass encoder FFN (ffn_h3.hip): y = LayerNorm(x + ReLU(x W1^T + b1) W2^T + b2) (eps 1e-5)
 * on fp32 x / y [M][256] (y may be x), F hidden units.  w1 = fp16 [2][F][ld1] hi, lo of W1[j] 2^e1_j;
 * meta1 = [F/32][64] floats: 2^-e1 of the chunk's 32 units, then their b1; w2 = fp16 [2][256][ld2]
 * hi, lo of W2[n] 2^e2_n with the columns of each 32-wide chunk permuted by spe_debug_ffn_h3_perm;
 * sinv2 = 2^-e2; amax_x = device bound on |x|; sh = the hidden activation's power-of-two scale. */
int spe_debug_ffn_h3(void* stream, const float* x, int ldx, float* y, int ldy, int M, int F, const void* w1, int ld1,
                     const float* meta1, const void* w2, int ld2, const float* sinv2, const float* b2,
                     const float* gamma, const float* beta, const float* amax_x, float sh);
/* position p (0..31) of a 32-wide hidden chunk in that column order -> the hidden unit it holds */
int spe_debug_ffn_h3_perm(int p);
/* the same launch with the weights also given pre-split (dtype SPE_DTYPE_F32X6_): planes = bf16
 * [3][plane_rows][ldb] holding hi, mid, lo of Bw (what spe_model_finalize writes for fp32x6 models) */
int spe_debug_gemm_planes(void* stream, int dtype, int mode, const void* A, int lda, const void* P, int ldp, int prow,
                          int H, int W, int Cin, int KH, int KW, int stride, int pad, const void* Bw, int ldb, int M,
                          int N, int K, const float* bias, const void* R, int ldr, int act_code, void* C, int ldc,
                          const void* planes, int plane_rows);
/* attention: dtype | 0x100 = V^T in the 16-bit DMA kernel's key order; dtype SPE_DTYPE_F32X3_ | 0x200 =
 * k and vt given as bf16 hi planes ([B*Tk][ldk] and [B][H][32][Tk]), each followed by its lo plane
 * (what the fp32x3 / fp32x6 models' projection epilogues write; Tk % 8 == 0); | 0x200 | 0x100 = those
 * planes with V^T in that key order (Tk % 16 == 0: the LDS-DMA split kernel, attn_split.hip), and
 * | 0x400 on top = the V^T planes as fp16 hi / lo (the fp32h3 model's form, here unscaled) (ABI 8) */
int spe_debug_attention(void* stream, int dtype, const void* q, int ldq, const void* k, int ldk, const void* vt,
                        void* o, int ldo, int B, int H, int Tq, int Tk, float scale);
/* the attention-map kernel (attn_map.hip) on caller operands: out[b][i][j] = (1/H) sum_h softmax_j(q_h[b][i] .
 * k_h[b][j] / sqrt(32)), fp32 [B][Tq][Tk]; q [B][H][Tq][32], k [B][H][Tk][32] of dtype BF16_ / F16_ / F32_, H = 8.
 * dtype BF16_ | 0x100: the bf16 decoder's folded cross-attention form, q' [B][Tq][8*256] already in the exp2
 * domain against one k [B][Tk][256] for every head: softmax_j of exp2(q'_h[b][i] . k[b][j]). */
int spe_debug_attn_map(void* stream, const void* q, const void* k, int B, int H, int Tq, int Tk, int dtype, float* out);
int spe_debug_layernorm(void* stream, int dtype, const void* x, const float* gamma, const float* beta, void* out,
                        float* out_f32, int M, int D);
/* ffn (bf16 only): y = LayerNorm(x + W2 relu(W1 x + b1) + b2), D == 256, F % 32 == 0; x and y may
 * alias.  W1 [F][ld1], W2 [D][ld2], biases / LayerNorm affine fp32.  partial (nullable, fp32
 * [splits][M][D]) selects the split-over-F form used for few rows (splits divides F/32).  ld2 == 0
 * (ABI 7 addition): W2 is chunk-packed [F/32][D][32], the bf16 model's encoder form. */
int spe_debug_ffn(void* stream, const void* x, int ldx, const void* w1, int ld1, const float* b1, const void* w2,
                  int ld2, const float* b2, const float* gamma, const float* beta, void* y, int ldy, int M, int D,
                  int F, float* partial, int splits);
/* the pre-norm forms of the two fused bf16 encoder kernels (SPE_MODEL_PRE_NORM).
 * ffn_pre: n = LayerNorm(x; gamma, beta) on chip (fp32 statistics, n rounded to bf16), y = x + W2 relu(W1 n + b1)
 * + b2 (bf16; x and y may alias), and beside it y2 = LayerNorm(y as stored; gamma2, beta2) (y2 nullable; row
 * stride ldy; not x) and, with pos ([pos_period][256] bf16) and ypos, ypos = y2 + pos[m % pos_period] (needs y2).
 * Other arguments as spe_debug_ffn.
 * oproj_pre: C = R + A . W^T + bias, bf16, K = N = 256, W [256][ldb], no LayerNorm; C may alias R. */
int spe_debug_ffn_pre(void* stream, const void* x, int ldx, const void* w1, int ld1, const float* b1, const void* w2,
                      int ld2, const float* b2, const float* gamma, const float* beta, void* y, int ldy, int M, int D,
                      int F, float* partial, int splits, const float* gamma2, const float* beta2, void* y2,
                      const void* pos, int pos_period, void* ypos);
int spe_debug_oproj_pre(void* stream, const void* A, int lda, const void* W, int ldb, const float* bias, const void* R,
                        int ldr, void* C, int ldc, int M);
/* xattn (bf16 only, the decoder cross-attention against the memory): for image b, query q and
 * head h, u[b*Q+q][h*256 .. +256] = softmax_t(q'[b*Q+q][h*256 ..] . k[b*T+t]) . v[b*T+t] with the
 * scores already in the exp2 domain (k = memory + pos, v = memory, rows of 256).  wv non-null
 * ([256][256] bf16, bv fp32): o[b*Q+q][h*32 + j] = wv[h*32 + j] . u_h + bv[h*32 + j] is written
 * instead of u.  splits <= 0 picks the launch's own key split; partial_scratch: fp32,
 * splits * B * 8Q * 258.  (ABI 7: the measured-negative shared-pos variant and its k_shared
 * argument are gone.) */
int spe_debug_xattn(void* stream, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* u,
                    int ldu, const void* wv, const float* bv, void* o, int ldo, int B, int Q, int T, int splits,
                    float* partial_scratch);
/* xattn_h3 (fp32h3, xattn_h3.hip, ABI 9 addition): the same cross-attention at fp32-level products --
 * q' fp32 [B*Q][ldq] (exp2 domain), mem fp32 [B*T][256], pos fp32 [T][256], keys mem + pos, values mem,
 * *mem_amax (device) >= max |mem|: mem is first written as fp16 hi / lo planes into plane_scratch
 * (B*T*2048 bytes), then o[b*Q+q][h*32 + j] = wv[h*32 + j] . u_h + bv[h*32 + j] (wv [256][256] fp32) is
 * written in fp32 and max |o| raised into *o_amax (nullable; an unsigned-max slot, zero it first).
 * splits <= 0: the launch's own key split; partial_scratch as spe_debug_xattn's. */
int spe_debug_xattn_h3(void* stream, const float* q, int ldq, const float* mem, const float* pos, const float* mem_amax,
                       const float* wv, const float* bv, float* o, int ldo, float* o_amax, int B, int Q, int T,
                       int splits, float* partial_scratch, void* plane_scratch);
/* upconv (bf16 models' neck, replaces the upsample + conv pair of REV/models/backbone.py:141
 * s16_latern(up16sto8s(xs16))): z [B*H*W][9*C] holds the per-tap products W_t . x at the low
 * resolution (t = kh*3 + kw); out [B][2H][2W] rows of stride ldo receive conv3x3(pad 1) of the
 * align_corners bilinear x2 upsample, i.e. sum over in-grid taps of the bilinear interpolation
 * of z's tap block.  C % 8 == 0 (bf16) / C % 4 == 0 (fp32). */
int spe_debug_upconv(void* stream, int dtype, const void* z, void* out, int ldo, int B, int H, int W, int C);
/* btail (bf16, the layer-1 bottleneck tail fused with the next block's conv1, btail.hip):
 * y [M][256] = relu(a [M][k1] . w3^T + b3 (+ r [M][256])), z [M][n2] = relu(y . w1p^T + b1) where
 * w1p [n2][256] holds conv1's columns in spe_debug_btail_perm order; (k1, n2, r) in
 * {(64, 64, r), (64, 128, r), (128, 64, null)}. */
int spe_debug_btail(void* stream, const void* a, int lda, int k1, const void* r, const void* w3, int ld3,
                    const float* b3, void* y, const void* w1p, int ld1, const float* b1, void* z, int n2, int M);
/* btail with every row stride and its two store forms chosen by the caller (additive, ABI 9; spe_debug_btail
 * follows the SPE_BTAIL_ROWS knob).  rows: 0 = r, y and z move as 8-byte row pieces, 1 = as 16-byte pieces
 * (strides then multiples of 8); w1p holds conv1's columns in spe_debug_btail_perm order either way.
 * H > 0 and W > 0 request the compact y store for M = B * H * W pixels: only the pixels with even h and
 * even w are stored, densely, as [B][H/2][W/2][256] with row stride ldy -- served for (k1, n2, r) = (64, 128, r),
 * even H and W and M a multiple of H * W; otherwise y is stored whole.  Returns 0 = launched, y whole;
 * 2 = launched, y compact; 1 = not served (nothing launched); < 0 = bad argument. */
int spe_debug_btail_rows(void* stream, const void* a, int lda, int k1, const void* r, int ldr, const void* w3, int ld3,
                         const float* b3, void* y, int ldy, const void* w1p, int ld1, const float* b1, void* z, int ldz,
                         int n2, int M, int rows, int H, int W);
/* btail_wide (bf16, the layer-2 / layer-3 bottleneck tail fused with the next block's conv1,
 * btail_wide.hip; additive, ABI 9): y [M][n1] (row stride ldy) = relu(a [M][k1] . w3^T + b3
 * (+ r [M][n1], row stride ldr)), z [M][n2] (row stride ldz) = relu(y . w1p^T + b1) where w1p
 * [n2][ld1] holds conv1's columns in spe_debug_btail_wide_perm(n1, .) order; (k1, n1, n2) in
 * {(128, 512, 128), (128, 512, 256), (256, 1024, 256)}, r nullable.  Returns 0, or 1 = not served
 * (another shape, or SPE_BTAIL_WIDE=0): nothing was launched. */
int spe_debug_btail_wide(void* stream, const void* a, int lda, int k1, const void* r, int ldr, const void* w3, int ld3,
                         const float* b3, void* y, int ldy, int n1, const void* w1p, int ld1, const float* b1, void* z,
                         int ldz, int n2, int M);
/* btail_wide's final form (additive, ABI 9): the same operands; relu_z = 0 leaves z = y . w1p^T + b1 without
 * the ReLU (the stride-16 DETR's input_proj over the last bottleneck), and y may be null: then y is not
 * stored at all (z is what it would be with y stored, bit for bit).  y null or relu_z = 0 are served for
 * (k1, n1, n2) = (256, 1024, 256) only.  Returns as spe_debug_btail_wide. */
int spe_debug_btail_wide_proj(void* stream, const void* a, int lda, int k1, const void* r, int ldr, const void* w3,
                              int ld3, const float* b3, void* y, int ldy, int n1, const void* w1p, int ld1,
                              const float* b1, void* z, int ldz, int n2, int M, int relu_z);
/* decsa (bf16 only, the decoder self-attention block, decsa.hip): in place over tgt [B*Q][ldt],
 * per image b: tgt = LayerNorm(tgt + MHA(q = k = tgt + query_pos, v = tgt) . wo^T + bo) with
 * 8 heads of 32 (d = 256), q|k = tgt . wqk^T + bqk + qpos ([Q][512] bf16, query_pos . wqk^T),
 * v = tgt . wv^T + bv, LayerNorm gamma g / beta b (eps 1e-5).  Q <= 64; weights bf16 rows. */
int spe_debug_decsa(void* stream, void* tgt, int ldt, int B, int Q, const void* wqk, int ldqk, const float* bqk,
                    const void* wv, int ldv, const float* bv, const void* qpos, const void* wo, int ldo,
                    const float* bo, const float* g, const float* b, float scale);
/* decproj (bf16 only, decsa.hip): in place over tgt [B*Q][ldt], tgt = LayerNorm(tgt + x . wo^T + bo)
 * per row (the decoder cross-attention's out-projection + norm2), x [B*Q][ldx] bf16, d = 256,
 * Q <= 64 (one workgroup per image). */
int spe_debug_decproj(void* stream, void* tgt, int ldt, const void* x, int ldx, int B, int Q, const void* wo, int ldo,
                      const float* bo, const float* g, const float* b);
/* decxproj (bf16 only, decsa.hip, ABI 7 addition): the cross-attention's tail in place over tgt:
 * merges the key-split partials spe_debug_xattn left in partial_scratch (same B, Q, T, splits),
 * o[b*Q+q][h*32 + j] = wv[h*32 + j] . u_h + bv[h*32 + j] rounded to bf16, then
 * tgt = LayerNorm(tgt + o . wo^T + bo) -- xattn's merge kernel and decproj as one launch, Q <= 48. */
int spe_debug_decxproj(void* stream, void* tgt, int ldt, float* partial_scratch, int splits, int T, int B, int Q,
                       const void* wv, int ldwv, const float* bv, const void* wo, int ldo, const float* bo,
                       const float* g, const float* b);
/* The decoder kernels (decsa, decproj, decxproj) read fragment-packed weights: bf16 rows
 * w [N][ld] (K = 256, N % 16 == 0) -> dst [N/16][8][64][8], lane l's A fragment of column tile t,
 * K-step ks at ((t*8 + ks)*64 + l)*8 (ABI 7 addition).  Their hooks take row-major weights with
 * ld > 0 (packed into scratch per call) or packed ones with ld == 0. */
int spe_debug_wfrag_pack(void* stream, const void* w, int ld, int N, void* dst);
/* decffn (bf16, decsa.hip + ffn.hip's reduce, ABI 7 addition): y [M][ldy] = LayerNorm(x + W2
 * relu(W1 x + b1) + b2) for few rows, d = 256, F % 256 == 0, through fp32 partials
 * [F/256][M][256]; x and y may alias.  w1 [F][ld1], w2 [256][ld2] row-major (or packed with ld 0:
 * w1 as spe_debug_wfrag_pack of [F] rows, w2 per 256-wide chunk of columns at chunk * 256 * 256). */
int spe_debug_decffn(void* stream, const void* x, int ldx, int M, int F, const void* w1, int ld1, const float* b1,
                     const void* w2, int ld2, const float* b2, const float* gamma, const float* beta, void* y, int ldy,
                     float* partial);
/* decq (bf16, decsa.hip, ABI 7 addition): y [M][ldy] = x . w^T + bias + r[m % period] over K = 256,
 * N % 256 == 0 (the decoder cross-attention's folded query projection); w [N][ldw] row-major or
 * packed with ldw 0; bias (fp32) and r (bf16 [period][ldr]) nullable. */
int spe_debug_decq(void* stream, const void* x, int ldx, int M, int N, const void* w, int ldw, const float* bias,
                   const void* r, int ldr, int period, void* y, int ldy);
/* the K-column order btail's second product expects: stored column k holds channel perm(k) */
int spe_debug_btail_perm(int k);
/* btail with 16-byte row pieces (additive, ABI 9): the weight row (output channel) that row p of the kernel's
 * image of w3 / w1p holds, so that MFMA fragment j leaves lane group fg, register r with channel
 * 32 (j / 2) + 8 sg + 4 (j % 2) + r, sg = (0, 2, 1, 3)[fg]; -1 for p < 0 */
int spe_debug_btail_row_perm(int p);
/* the same for btail_wide at block-output width n1 (512 / 1024); -1 outside [0, n1) */
int spe_debug_btail_wide_perm(int n1, int k);
/* stempool (bf16, stempool.hip): out [B][Po][Po] rows of stride ldo (Po = S/4 for S % 4 == 0) =
 * maxpool3x3/s2/p1(relu(conv7x7/s2/p3(image) + bias)) from x = the zero-bordered pair-packed
 * input [B][S+6][S+6][4] and w [64][ldw] with k = (kh*8 + kw)*4 + ci (registry.cpp's stem). */
int spe_debug_stempool(void* stream, const void* x, const void* w, int ldw, const float* bias, void* out, int ldo,
                       int B, int S);

/* MobileNetV3_Large backbone kernels (mbv3.hip, ABI 9 additions; act: 0 none, 1 ReLU, 4 Hardswish).
 * dwconv: depthwise k x k conv, pad k/2, over NHWC x [B][H][W][C] -> y [B][Ho][Wo][C], y = act(conv + bias);
 * w fp32 [k*k][C] (tap-major, a folded BatchNorm scale included), bias fp32 [C]; dtype BF16_ (fp32
 * accumulation) or F32_.  Contract, checked before any launch (SPE_E_ARG): k 3 or 5; stride 1, or 2 with
 * even H and W (Ho = H / stride, Wo = W / stride); C % 8 == 0; B <= 65535.  pool_partials (nullable): fp32
 * [B][spe_debug_dwconv_tiles(Ho, Wo)][C], per 8 x 8 output tile the sum of the stored outputs, added in a
 * fixed order (no floating-point atomics: two runs give the same bits) -- the SE gate's pool. */
int spe_debug_dwconv_tiles(int Ho, int Wo);
int spe_debug_dwconv(void* stream, int dtype, const void* x, const float* w, const float* bias, void* y,
                     float* pool_partials, int B, int H, int W, int C, int k, int stride, int act);
/* se_gate: scale [B][C] = hardsigmoid(w2 . relu(w1 . mean + b1)), mean[b][c] = inv_hw * sum_t
 * pool_partials[b][t][c]; w1 fp32 [hidden][C] (the BatchNorm folded in), b1 [hidden], w2t fp32 [hidden][C]
 * (the second conv's [C][hidden] weight transposed).  fp32 in both model dtypes.  C <= 1024, hidden <= 256. */
int spe_debug_se_gate(void* stream, const float* pool_partials, int tiles, float inv_hw, const float* w1, const float* b1,
                      const float* w2t, float* scale, int B, int C, int hidden);
/* pwconv: c [M][ldc] = act((a . scale) . w^T + bias + r): a [M][lda], w [N][ldw], r [M][ldr] (nullable) and c
 * in dtype (BF16_: MFMA bf16, fp32 accumulation; F32_: exact-f32 MFMA); bias fp32 [N] (nullable); scale fp32
 * [M / rows_per_image][K] (nullable): row m's a is multiplied by scale[m / rows_per_image] and rounded to
 * dtype; the residual is added BEFORE the activation.  N, K, lda, ldw, ldc, ldr multiples of 8 (SPE_E_ARG). */
int spe_debug_pwconv(void* stream, int dtype, const void* a, int lda, const void* w, int ldw, const float* bias,
                     const float* scale, int rows_per_image, const void* r, int ldr, void* c, int ldc, int M, int N,
                     int K, int act);
/* The backbone stage alone of a finalized RT-DETR handle of either family (what spe_rtdetr_forward runs
 * first): images as spe_rtdetr_forward's; f0 / f1 / f2 = the stride 8 / 16 / 32 maps as fp32 NCHW
 * [B][C_l][S/8 .. S/32]^2 (C_l = 128, 256, 512, x 4 for depth 50). */
int spe_debug_rtdetr_backbone(spe_model* m, void* stream, const float* images, int batch, void* workspace,
                              int64_t workspace_bytes, float* f0, float* f1, float* f2);
/* mb_stem: the MobileNetV3 stem alone, conv1 3x3/s2/p1 3 -> 16 + bias + Hardswish -> NHWC y [B][S/2][S/2][16].
 * Source: images (fp32 NCHW [B][3][S][S]) or, when crops is not null, 8-bit crops [B][S][S][channels]
 * (channels 1 / 3; 4-byte aligned, S % 32 == 0).  w fp32 [27][16] with k = (ci*3 + kh)*3 + kw, bias fp32 [16]. */
int spe_debug_mb_stem(void* stream, int dtype, const float* images, const void* crops, int channels, const float* w,
                      const float* bias, void* y, int B, int S);
/* mbs_entry (mbv3s.hip): the MobileNetV3_Small entry in one launch, from the same two sources (crops need no
 * alignment here) to three NHWC maps [B][S/4][S/4][16] of dtype: pooled = the 2 x 2 mean of the stem map,
 * skip = dw3x3/s2(stem) + bias, t2 = relu(dw3x3/s2(relu(stem . We + be)) + bias); the stem map and the expanded
 * map are zero outside [0, S/2)^2 (the reference's padding).  pool_partials (nullable): fp32
 * [B][spe_debug_mbs_entry_tiles(S)][16], per 8 x 8 tile the sum of the stored t2 values in a fixed order.
 * weights: fp32 [1040], BatchNorm folded: stem [27][16], bias [16], expand [ci][co] 256, bias 16, depthwise
 * [9][16], bias 16, skip depthwise [9][16], bias 16.  S a multiple of 16, 32 <= S <= 4096 (SPE_E_ARG otherwise). */
int spe_debug_mbs_entry_tiles(int S);
int spe_debug_mbs_entry(void* stream, int dtype, const float* images, const void* crops, int channels,
                        const float* weights, void* pooled, void* skip, void* t2, float* pool_partials, int B, int S);

/* GhostNetV2 backbone kernels (ghostv2.hip, ABI 9 additions).  Every refusal below is SPE_E_ARG before any
 * launch; dtype BF16_ (fp32 accumulation) or F32_.
 * ghost_cheap: the second half of a ghost module and what follows it.  x1 is a channel slice of an NHWC
 * tensor: pixel (b, h, w) at x1 + ((b*H + h)*W + w)*ldx + xoff, `half` channels.  x2 = act(dw3x3(x1) + bias)
 * (pad 1; w fp32 [9][half] tap-major with the BatchNorm scale folded in, bias fp32 [half]; act 0 none or 1
 * ReLU).  y [B][H][W][2*half]: y[:half] = post(x1), y[half:] = post(x2) with post 0 nothing, 1 multiply by
 * gate[b][h/2][w/2][c] (dtype [B][H/2][W/2][2*half]; H and W even) -- the gate applies to the activated
 * concat, the depthwise conv reads the ungated x1 --, 2 add resid[b][h][w][c] (dtype, y's layout).
 * pool_partials (nullable): fp32 [B][spe_debug_dwconv_tiles(H, W)][2*half], per 8 x 8 tile the sum of the
 * stored outputs in a fixed order (two runs give the same bits).  Contract: half, ldx, xoff multiples of 8
 * (a narrower half is stored padded to 8 with zero weights and bias: its pad lanes come out exactly 0),
 * ldx >= xoff + half, B <= 65535, y not aliasing x1. */
int spe_debug_ghost_cheap(void* stream, int dtype, const void* x1, int ldx, int xoff, const float* w, const float* bias,
                          void* y, const void* gate, const void* resid, float* pool_partials, int B, int H, int W,
                          int half, int act, int post);
/* dfc_gate: gate = sigmoid(dw5x1(dw1x5(x) + b1) + b2) over NHWC x [B][H][W][C] -> gate, same shape; w1 / w2
 * fp32 [5][C] (tap-major: w1 along W, pad 2; w2 along H, pad 2), b1 / b2 fp32 [C]; no activation or rounding
 * between the two convs.  Contract: H, W <= 32 (the whole map sits in LDS), C % 8 == 0, B <= 65535. */
int spe_debug_dfc_gate(void* stream, int dtype, const void* x, const float* w1, const float* b1, const float* w2,
                       const float* b2, void* gate, int B, int H, int W, int C);
/* se_gate_bias: spe_debug_se_gate with the second conv's bias b2 fp32 [C] added before the Hardsigmoid. */
int spe_debug_se_gate_bias(void* stream, const float* pool_partials, int tiles, float inv_hw, const float* w1,
                           const float* b1, const float* w2t, const float* b2, float* scale, int B, int C, int hidden);
/* pool2: 2 x 2 mean, NHWC x [B][H][W][C] -> y [B][H/2][W/2][C]; H, W even, C % 8 == 0. */
int spe_debug_pool2(void* stream, int dtype, const void* x, void* y, int B, int H, int W, int C);

/* RT-DETR kernels (rtdetr.hip, ABI 9 additions): each hook fills the kernel's argument struct and returns the
 * launcher's own code: 0, a hipError_t, or -5 when the arguments are outside the kernel's contract (refused
 * before any launch; spe_last_error is not set).  dtype BF16_ or F32_ is the type T of the buffers marked T;
 * everything else is fp32.  A channel slice of a wider buffer is passed as the pointer of its first column.
 * rt_resample2x: NHWC in [B][H][W][ldi] T -> out [B][Ho][Wo][ldo] T over C channels; mode 0 nearest x2, mode 1
 * bicubic x0.5 (align_corners=False, a = -0.75, clamped taps; H and W even).  C, ldi, ldo multiples of the
 * 16-byte chunk (8 bf16, 4 fp32). */
int spe_debug_rt_resample2x(void* stream, int dtype, const void* in, int ldi, void* out, int ldo, int B, int H, int W,
                            int C, int mode);
/* rt_query_select: per image the Q tokens of highest max-over-classes logit, descending, the lower token index
 * first among equal scores.  Rows are level-major: token t of level l of image b is row B*lvl_start[l] +
 * b*hw_l + (t - lvl_start[l]); lvl_start (host) has levels + 1 entries, the last one L.  logits [rows][C],
 * memory [rows][ldm] T (D columns gathered), anchors [L][2] -> topk [B][Q] int32, target [B*Q][ldt] T,
 * sel_logits [B*Q][C], sel_anchors [B*Q][2].  1 <= levels <= 4, L <= 12288, 1 <= Q <= min(64, L), 1 <= C <= 256. */
int spe_debug_rt_query_select(void* stream, int dtype, const float* logits, int C, const void* memory, int ldm,
                              const float* anchors, int B, int Q, int D, int levels, const int* lvl_start, int* topk,
                              void* target, int ldt, float* sel_logits, float* sel_anchors);
/* rt_qpos_hidden: out [rows][H] T = relu(ref [rows][2] . w0 [H][2]^T + b0 [H]). */
int spe_debug_rt_qpos_hidden(void* stream, int dtype, const float* ref, const float* w0, const float* b0, void* out,
                             int rows, int H);
/* rt_head_finish: the last layers of the score / box / sigma heads and the post-processor, per query row:
 * logits = hs [rows][256] . cls_w [C][256]^T + cls_b, probs = softmax(logits) (cls_w null: no score head, both
 * untouched; probs nullable); points = sigmoid(h2[:256] . box_w2 [2][256]^T + box_b2 + add), add = pt_add
 * [rows][2] or inverse_sigmoid(pt_add) (pt_add_invsig 1); points_px = points * (x1 - x0, y1 - y0) + (x0, y0)
 * with clip_bbox [rows / Q][4] (both nullable); log_sigmas = h2[256:512] . sig_w2 [256] + sig_b2 repeated to 2
 * columns, sigmas = exp of it (sig_w2 null: no sigma head; both nullable).  h2 [rows][ld_h2] T.  C <= 16;
 * points, pt_add, h2 required; a score head needs hs and logits. */
int spe_debug_rt_head_finish(void* stream, int dtype, int rows, int Q, int C, const float* hs, const float* cls_w,
                             const float* cls_b, const void* h2, int ld_h2, const float* box_w2, const float* box_b2,
                             const float* sig_w2, const float* sig_b2, const float* pt_add, int pt_add_invsig,
                             float* logits, float* probs, float* points, const float* clip_bbox, float* points_px,
                             float* log_sigmas, float* sigmas);
/* rt_msdeform: the multi-scale deformable attention core.  value T: level-major rows lvl_rows0[l] + b*H_l*W_l +
 * y*W_l + x of ldv columns, 256 read (head h, channel c at h*32 + c); so_aw [rows][ld_so]: heads*levels*points
 * (x, y) offsets, then heads*levels*points attention logits; ref [rows][2]; out [rows][ldo] T; image of a row =
 * row / Q.  lvl_h, lvl_w, lvl_rows0 (host) have `levels` entries.  heads 8, levels <= 4, points <= 4. */
int spe_debug_rt_msdeform(void* stream, int dtype, const void* value, int ldv, const float* so_aw, int ld_so,
                          const float* ref, void* out, int ldo, int rows, int Q, int heads, int levels, int points,
                          const int* lvl_h, const int* lvl_w, const int* lvl_rows0);
/* rt_deform_map: the head-averaged attention map of one rt_msdeform call (spe_rtdetr_forward_attention's decoder
 * tap) from the same so_aw / ref / level sizes; it reads no value, so it has no dtype.  map [rows][L] (L = sum of
 * H_l * W_l, columns level-major, y * W_l + x; cells no sample touches are exactly 0), loc [rows][heads][levels]
 * [points][2], weights [rows][heads][levels][points]: each nullable, not all three.  No atomics and a fixed
 * summation order: two runs are bit-identical.  heads 8, 1 <= levels <= 4, 1 <= points <= 4, L <= 12288. */
int spe_debug_rt_deform_map(void* stream, const float* so_aw, int ld_so, const float* ref, int rows, int Q, int heads,
                            int levels, int points, const int* lvl_h, const int* lvl_w, float* map, float* loc,
                            float* weights);

/* DETR stem, neck and head helpers (elementwise.hip, heads.hip; additions, ABI 9 unchanged).  As the rt hooks:
 * the launcher's own code, 0, a hipError_t, or -5 / -6 when the arguments are outside the kernel's contract
 * (refused before any launch; spe_last_error is not set); a null required pointer is SPE_E_ARG.
 * pack_input: the crop batch, images_f32 [B][3][S][S] or (when that is null) crops_u8 [B][S][S][channels]
 * (channels 1: gray into all three, or 3; normalised (u / 255 - mean) / std in fp32) -> NHWC out [B][S][S][cpad]:
 * dtype BF16_ cpad 8, F32_ cpad 8 or 4; the pad channels are +0.  amax (nullable, F32_ only; BF16_ ignores it):
 * one fp32 slot raised to max |x| when that is larger, never lowered.  Neither source, or channels not 1 / 3: -5. */
int spe_debug_pack_input(void* stream, int dtype, const float* images_f32, const void* crops_u8, int channels, void* out,
                         int B, int S, int cpad, float* amax);
/* pack_input_pad4: the same sources -> bf16 out [B][S+6][S+6][4], the image inside a 3-pixel border; the border
 * and channel 3 are written as zeros on every call. */
int spe_debug_pack_input_pad4(void* stream, const float* images_f32, const void* crops_u8, int channels, void* out, int B,
                              int S);
/* maxpool3s2: 3 x 3 / stride 2 / pad 1 max-pool (-inf padding), NHWC in [B][H][W][C] T -> out [B][Ho][Wo] rows of
 * stride ldo T (0 = C; a channel slice of a concat buffer), Ho = (H - 1) / 2 + 1, Wo likewise.  C and ldo
 * multiples of the 16-byte chunk (8 bf16, 4 fp32), ldo >= C, else -5. */
int spe_debug_maxpool3s2(void* stream, int dtype, const void* in, void* out, int B, int H, int W, int C, int ldo);
/* upsample2x: bilinear x2, align_corners=True, NHWC in [B][H][W][C] T -> out [B][2H][2W][C] T; C a multiple of
 * the 16-byte chunk, else -5. */
int spe_debug_upsample2x(void* stream, int dtype, const void* in, void* out, int B, int H, int W, int C);
/* heads: the class / point / sigma heads fused with PostProcess on hs [B*Q][256] fp32, D == 256 (else -6);
 * weights transposed [in][out] as the kernel reads them: cls_wt [256][12], pt_w0t / pt_w1t [256][256], pt_w2t
 * [256][2], sg_* the same with sg_w2t [256][1] (sg_w0t null: no sigma head).  logits [B*Q][12], points [B*Q][2]
 * (sigmoid); probs (nullable) softmax; points_px (nullable, needs clip_bbox [B][4]) = points * (x1 - x0, y1 - y0)
 * + (x0, y0) of image row / Q; log_sigmas, sigmas (nullable) [B*Q][2], both columns equal.  B * Q == 0: 0. */
int spe_debug_heads(void* stream, const float* hs, int B, int Q, int D, const float* cls_wt, const float* cls_b,
                    const float* pt_w0t, const float* pt_b0, const float* pt_w1t, const float* pt_b1, const float* pt_w2t,
                    const float* pt_b2, const float* sg_w0t, const float* sg_b0, const float* sg_w1t, const float* sg_b1,
                    const float* sg_w2t, const float* sg_b2, const float* clip_bbox, float* logits, float* points,
                    float* probs, float* points_px, float* log_sigmas, float* sigmas);
/* groupnorm: GroupNorm(32, C), eps 1e-5, over NHWC rows x [B*H*W][ldx] T (dtype BF16_ or F32_):
 * y = (x - mean) * rsqrt(var + eps) * gamma[c] + beta[c] (+ residual) (ReLU when relu != 0), mean and biased variance
 * per (image, group of C / 32 consecutive channels), fp32 statistics from the stored values.  Runs the model's two
 * launches (stats, then apply) with `scratch` holding the partial statistics, fp32 [B][tiles][32][3] (count, mean,
 * M2): spe_debug_groupnorm_scratch_bytes(B, H, W, C) = B * tiles * 384 bytes (0 for sizes it does not serve), tiles =
 * ceil(H * W / (16384 / C)) for both dtypes.  x, residual and y may alias.  SPE_E_ARG before any launch: C not a
 * multiple of 32 (or C / 32 not 2, 4, 8, 16 or 32), an ld below C or not a multiple of 8, a null x / gamma / beta / y /
 * scratch, a pointer not 16-byte aligned, scratch_bytes below the stated size. */
int spe_debug_groupnorm(void* stream, int dtype, const void* x, int ldx, const void* residual, int ldr,
                        const float* gamma, const float* beta, void* y, int ldy, int B, int H, int W, int C, int relu,
                        void* scratch, int64_t scratch_bytes);
int64_t spe_debug_groupnorm_scratch_bytes(int B, int H, int W, int C);

#ifdef __cplusplus
}
#endif
#endif
