// Internal launcher interface between the C++ runtime (model.cpp, pnp host code) and the HIP
// kernels.  Not part of the public C ABI (include/spe.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

enum { SPE_DTYPE_BF16 = 0, SPE_DTYPE_F32 = 1, SPE_DTYPE_F16 = 2,    // F16: attention operands only
       SPE_DTYPE_BF16_F16V = 3,     // attention only: bf16 q/k, fp16 V^T and P (bf16 models' encoder)
       SPE_DTYPE_F32X3 = 4,         // fp32 storage, split-bf16 (hi.hi + hi.lo + lo.hi) MFMA compute
       SPE_DTYPE_F32X6 = 5,         // fp32 storage, three-way split-bf16 (6 products, ~fp32) MFMA compute (GEMMs)
       SPE_DTYPE_F32H3 = 6 };       // fp32 storage, scaled two-way split-fp16 (3 products, ~fp32) MFMA compute (GEMMs)
enum { GEMM_LINEAR = 0, GEMM_LINEAR_ADD = 1, GEMM_CONV = 2 };
// GEMM epilogue activations: ReLU (ResNet, DETR FFN), SiLU (UNC hybrid encoder ConvNormLayer,
// hybrid_encoder.py:17-37), exact-erf GELU (UNC AIFI FFN, torch nn.GELU default)
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_SILU = 2, ACT_GELU = 3 };

struct GemmArgs {
  const void* A; int lda;          // LINEAR*: A[m*lda + k]; CONV: NHWC input [B][H][W][Cin]
  const void* P; int ldp; int prow;// LINEAR_ADD: A += P[(m % prow)*ldp + k]
  int H, W, Cin, KH, KW, stride, pad, Ho, Wo;   // CONV geometry
  const void* B; int ldb;          // weights [N][ldb], ldb % 64 == 0
  int M, N, K;
  const float* bias;               // [N] or null
  const void* R; int ldr;          // residual [m*ldr + n] or null
  int act;                         // ACT_*: y = act(acc + bias + R), or act(acc + bias) + R
  int res_post;                    //   with res_post (CSPRepLayer's silu(rep(x1)) + x2)
  void* C; int ldc;                // output [m*ldc + n]
  int out_f32;                     // store fp32 instead of T
  int out_f16;                     // bf16 models: store fp16 instead of bf16 (fp16 attention operands)
  int vt_T, vt_B;                  // >0: head-transposed store (see gemm.hip)
  int vt_swz;                      // head-transposed 16-bit store with the attention's key order: within
                                   // each 16-token group the middle quads swap (vt_pos; vt_T % 16 == 0)
  int r_period;                    // >0: residual row = m % r_period (row-periodic add, e.g. pos . W^T)
  const float* ln_g; const float* ln_b;   // optional fused post-norm LayerNorm over N == 256 (bf16, large M)
  const void* B6; int b6_rows;     // fp32x6: the weights pre-split into bf16 planes [3][b6_rows][ldb] (h, m, l), or null
  void* S; int s_col0;             // fp32 models: columns n >= s_col0 stored instead as bf16 hi / lo planes for the
                                   // fp32x3 attention: rows -> hi [M][N - s_col0] then lo; head-transposed
                                   // (vt_T) -> hi in C's layout [vt_B][N][vt_T] then lo (s_col0 = 0)
  // fp32h3 (gemm.hip gemm_h3d): the weights as fp16 planes [2][h3_rows][ldb] (hi, lo of W[n] * 2^e_n)
  // with h3_sinv[n] = 2^-e_n; amax_a: device max |A| (the A operand's scale 2^13 / amax rounded to
  // a power of two; null = 1).  amax_c (fp32 GEMMs): max |stored output| * (amax_c_mul or 1) is
  // atomically maxed into *amax_c (float bits as uint, >= 0) -- the next GEMM's amax_a
  const void* H3; int h3_rows; const float* h3_sinv;
  const float* amax_a;
  float* amax_c; float amax_c_mul;
  // head-transposed S planes as fp16 instead of bf16 (the fp32h3 encoder attention's value operand):
  // hi / lo of x * vplane_scale(amax_a, s_l1, s_bmax), s_l1 = max_n sum_k |W[n][k]|, s_bmax = max |bias|
  int s_f16; float s_l1, s_bmax;
};
bool spe_gemm_ln_fusable(const GemmArgs& g);   // the large-tile kernel can fuse ln_g/ln_b for g
int spe_launch_gemm(const GemmArgs& g, int dtype, int mode, hipStream_t s);
// the fp32h3 kernels only: 1 (nothing launched) for a shape they do not serve, where spe_launch_gemm
// would fall through to the x6 path
int spe_launch_gemm_h3(const GemmArgs& g, int mode, hipStream_t s);

// Implicit-GEMM conv K order.  Multi-tap convs with Cin % 64 == 0 use channel-block-major order
// k = ((ci / 64) * KH*KW + tap) * 64 + ci % 64, so one 64-channel slice of the input window is
// reused by all taps in consecutive K-steps (L2-resident) instead of the whole Cin-deep window
// being streamed once per tap; other convs use k = tap * Cin + ci.  Weights are packed to match
// (registry.cpp make_conv).
__host__ __device__ inline bool conv_channel_blocked(int Cin, int taps) { return (Cin & 63) == 0 && taps > 1; }
__device__ __forceinline__ void conv_k_decode(int k, int Cin, int KW, int taps, int& kh, int& kw, int& ci) {
  int tap;
  if (conv_channel_blocked(Cin, taps)) {
    const int cb = k / (64 * taps), rem = k - cb * 64 * taps;
    tap = rem >> 6;
    ci = cb * 64 + (rem & 63);
  } else {
    tap = k / Cin;
    ci = k - tap * Cin;
  }
  kh = tap / KW;
  kw = tap - kh * KW;
}
// Bottleneck tail + next conv1 (btail.hip): y = relu(A . W3^T + b3 (+ R)), z = relu(y . W1p^T + b1)
// with W1p's columns in spe_btail_perm order.  bf16; N1 = n1 = 256 (layer 1, btail.hip: both weight
// matrices in LDS) or 512 / 1024 (layers 2 / 3, btail_wide.hip: weights streamed in chunks, W1p's
// columns in spe_btail_wide_perm order).
struct BtailArgs {
  const void* A; int lda; int k1;        // conv3 input [M][k1] (row stride lda)
  const void* R; int ldr;                // residual [M][n1] or null
  const void* w3; int ld3; const float* b3;   // [n1][ld3]
  void* y; int ldy; int n1;              // block output [M][n1]
  const void* w1; int ld1; const float* b1;   // next conv1, permuted columns [n2][ld1]
  void* z; int ldz; int n2;              // next conv1 output [M][n2]
  int M;
  // btail.hip only.  rows: R, y and z move as 16-byte row pieces instead of 8-byte ones (same results).
  // ycompact: y's only reader is a stride-2 1x1 conv over the M = B*H*W pixels, so y is stored as the dense [B][H/2][W/2][n1] of the even pixels (row stride ldy) where
  // spe_btail_ycompact_serves, else whole.
  int rows, ycompact, H, W;
};
int spe_launch_btail(const BtailArgs& a, hipStream_t s);   // 1 = not applicable
int spe_btail_perm(int k);
// rows: the weight row (output channel) that row p of W3's and W1's LDS image holds.  MFMA fragment j
// (rows 16 j .. 16 j + 15) leaves lane group fg, register r with row 16 j + 4 fg + r, i.e. with channel
// 32 (j / 2) + 8 sg + 4 (j % 2) + r, sg = fg with its two bits swapped (0, 2, 1, 3): the fragment pair
// (2i, 2i + 1) gives a lane 8 consecutive channels (btail.hip's header: why sg and not fg)
__host__ __device__ inline int spe_btail_row_perm(int p) {
  return (p & ~31) | (((p >> 2) & 1) << 4) | (((p >> 3) & 1) << 3) | (((p >> 4) & 1) << 2) | (p & 3);
}
bool spe_btail_enabled();
bool spe_btail_rows_enabled();                    // SPE_BTAIL_ROWS (default 1)
bool spe_btail_ycompact_enabled();                // SPE_BTAIL_YCOMPACT (default 1)
bool spe_btail_ycompact_serves(const BtailArgs& a);   // what spe_launch_btail stores compactly
// the wide form: (k1, n1, n2) in {(128, 512, 128), (128, 512, 256), (256, 1024, 256)}; 1 = not served
// (another shape, or SPE_BTAIL_WIDE=0)
int spe_launch_btail_wide(const BtailArgs& a, hipStream_t s);
int spe_btail_wide_perm(int n1, int k);
bool spe_btail_wide_enabled();
bool spe_btail_wide_serves(const BtailArgs& a);   // what spe_launch_btail_wide launches
int spe_btail_wide_tiles(const BtailArgs& a);     // its grid (row tiles) for a served problem
// the final form, (k1, n1, n2) = (256, 1024, 256) only: z = y . W1p^T + b1 without the ReLU unless relu_z,
// and y not stored when a.y is null (the stride-16 DETR's last bottleneck -> input_proj); 1 = not served
int spe_launch_btail_wide_proj(const BtailArgs& a, bool relu_z, hipStream_t s);
bool spe_btail_wide_proj_serves(const BtailArgs& a);
bool spe_btail_wide_proj_enabled();               // SPE_BTAIL_PROJ=1: the model takes it (A/B knob; default 0)
int spe_launch_gemm2(const GemmArgs& g, int mode, hipStream_t s);   // 1 = not applicable
int spe_launch_sgemm(const GemmArgs& g, int mode, hipStream_t s);   // 1 = not applicable
int spe_launch_lnproj(const GemmArgs& g, hipStream_t s);             // 1 = not applicable (lnproj.hip)
bool spe_lnproj_applies(const GemmArgs& g);
// the pre-norm form C = R + A . W^T + b (no LayerNorm; in place over R allowed), same return convention
int spe_launch_lnproj_pre(const GemmArgs& g, hipStream_t s);
bool spe_lnproj_pre_applies(const GemmArgs& g);
// bf16 GEMM + residual + LayerNorm in one launch: lnproj.hip at any row count, else the large-tile kernel
inline bool spe_ln_fusable(const GemmArgs& g) { return spe_lnproj_applies(g) || spe_gemm_ln_fusable(g); }
int spe_launch_pconv(const GemmArgs& g, hipStream_t s);             // 1 = not applicable (pconv.hip)
int spe_cu_count();               // CUs of the current device (cached; 256 on MI355X)
// kernel family of this thread's last spe_launch_gemm: 0 gemm.hip, 1 gemm2.hip, 2 gemm_stream.hip,
// 3 pconv.hip
extern thread_local int spe_gemm_last_path;

// Stored position of token t in a vt_swz V^T row: bits 2 and 3 swap (quads 0, 2, 1, 3 of every
// 16 tokens), the key order the attention's P^T operand has straight out of its S^T accumulator.
__host__ __device__ inline int vt_pos(int t) { return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1); }

struct AttnArgs {
  const void* q; int ldq;          // query row b*Tq+i, head h at columns [h*32, h*32+32)
  const void* k; int ldk;          // key row b*Tk+j
  const void* vt;                  // V^T [B][H][32][Tk]
  int vt_swz;                      // V^T rows in vt_pos order (16-bit operands, Tk % 16 == 0): the
                                   // encoder kernel then stages K / V^T by LDS DMA
  void* o; int ldo;                // output row b*Tq+i
  int B, H, Tq, Tk;
  float scale;                     // softmax scale (1/sqrt(head_dim))
  int presplit;                    // fp32x3: k and vt are bf16 hi planes (k [B*Tk][ldk], vt [B][H][32][Tk]),
                                   // each followed by its lo plane (GemmArgs::S); Tk % 8 == 0.  With vt_swz
                                   // (V^T in vt_pos order, Tk % 16 == 0) the LDS-DMA split kernel (attn_split.hip)
  int v_f16;                       // presplit + vt_swz: the V^T planes are fp16 hi / lo of V * vplane_scale(
  const float* v_amax; float v_l1, v_bmax;   //   v_amax, v_l1, v_bmax) (GemmArgs::s_f16), P split to fp16
};
int spe_launch_attention_split(const AttnArgs& a, hipStream_t s);
int spe_launch_attention(const AttnArgs& a, int dtype, hipStream_t s);

// Head-averaged attention probabilities (attn_map.hip, the diagnostic tap of spe_forward_attention):
// out[b][i][j] = (1/8) sum_h softmax_j(scale q_h[b][i] . k_h[b][j]), fp32 [B][Tq][Tk].  Strides in
// elements; dtype SPE_DTYPE_BF16 / _F16 / _F32 is the storage of q and k.
struct AttnMapArgs {
  const void* q; long long q_sb, q_sh; int ldq;   // q_h[b][i] at q + b q_sb + h q_sh + i ldq, head_dim elements
  const void* k; long long k_sb, k_sh; int ldk;   // k_h[b][j] likewise (k_sh = 0: one k for every head)
  float* out;
  int B, H, Tq, Tk;                // H == 8
  int head_dim;                    // 32, or 256 (bf16, base2: the folded decoder cross-attention, xattn.hip)
  float scale;                     // softmax scale (ignored with base2)
  int base2;                       // q pre-scaled by scale . log2 e: softmax_j of exp2(q . k)
};
int spe_launch_attn_map(const AttnMapArgs& a, int dtype, hipStream_t s);   // -1: arguments outside the contract

// Decoder cross-attention against the encoder memory (bf16 path, xattn.hip): per image b and
// attention row r = q * 8 + h, u[b][q][h] = softmax(q'[b][q][h] . K^T) . V with K = memory +
// pos [T][256], V = memory [T][256], q' pre-scaled into the exp2 domain.
struct XattnArgs {
  const void* q; int ldq;          // q' rows b*Q + q, head h at columns [h*256, h*256 + 256)
  const void* k; int ldk;          // memory + pos, rows b*T + t
  const void* v; int ldv;          // memory, rows b*T + t
  void* u; int ldu;                // output rows b*Q + q, head h at columns [h*256, h*256 + 256)
  const void* wv; const float* bv; // optional: o_h = Wv_h u_h + bv_h written instead of u
  void* o; int ldo;                //   o rows b*Q + q, head h at columns [h*32, h*32 + 32)
  int B, Q, T, splits, tiles_per_split;
  float *pm, *pl, *pu;             // key-split partials [B][splits][8Q] (pu: x 256), required
  bool partials_only;              // stop at the partials (decproj's merge form consumes them)
  // fp32h3 (xattn_h3.hip): q' fp32; k / v the fp16 planes [B*T][512] (hi | lo) written by
  // spe_launch_xattn_h3_split from a memory bounded by *mem_amax; wv / bv / o fp32; max |o| raised into
  // *o_amax (the out-projection GEMM's scale input)
  const float* mem_amax; float* o_amax;
};
int spe_xattn_splits(int B, int Q, int T);
int spe_xattn_launch_splits(int T, int splits);   // the split count a launch with `splits` runs (partials' layout)
int spe_launch_xattn(const XattnArgs& a, hipStream_t s);
// fp32h3: kp = fp16 hi | lo of (mem + pos) * 2^sk, vp = of mem * 2^sv (powers of two from *mem_amax,
// vplane_scale), rows b*T + t of 512 halves; mem [B*T][256] fp32, pos [T][256] fp32
int spe_launch_xattn_h3_split(const float* mem, const float* pos, const float* mem_amax, void* kp, void* vp, int B,
                              int T, hipStream_t s);
int spe_launch_xattn_h3(const XattnArgs& a, hipStream_t s);

// Decoder self-attention block (bf16 only, decsa.hip), one workgroup per image, in place over tgt:
// tgt = LN(tgt + SelfAttn(q = k = tgt + qpos, v = tgt) . Wo^T + bo), 8 heads of 32, d = 256.
// The decoder kernels' weights are fragment-packed (spe_launch_wfrag_pack): [N/16][8][64][8] bf16,
// the 16-byte MFMA A fragment of lane l for column tile t and K-step ks at ((t*8 + ks)*64 + l)*8.
struct DecSaArgs {
  void* tgt; int ldt;              // [B*Q][ldt] bf16
  int B, Q;                        // Q <= 64
  const void* wqk; const float* bqk;   // in_proj rows 0..511 (packed), bias fp32
  const void* wv; const float* bv;     // in_proj rows 512..767 (packed)
  const void* qpos;                // [Q][512] bf16: query_pos . Wqk^T
  const void* wo; const float* bo;     // out_proj (packed)
  const float* g; const float* b;  // norm1
  float scale;                     // 1/sqrt(head_dim)
};
int spe_launch_decsa(const DecSaArgs& a, hipStream_t s);   // 1 = not applicable
// tgt = LN(tgt + x . Wo^T + bo), one workgroup per image (decsa.hip; bf16, d = 256, Q <= 64)
struct DecProjArgs {
  void* tgt; int ldt;              // [B*Q][ldt] bf16, in place
  const void* x; int ldx;          // [B*Q][ldx] bf16
  int B, Q;
  const void* wo; const float* bo; // out_proj (packed)
  const float* g; const float* b;
  // merge form (pm set, Q <= 48): x is the cross-attention's output computed here from xattn's
  // key-split partials (XattnArgs::partials_only) -- o_h = Wv_h u_h + bv_h, heads of 32
  const float *pm, *pl, *pu; int splits;
  const void* wv; const float* bv; // value rows of in_proj (packed)
};
// The decoder FFN's split-F product (decsa.hip, bf16, d = 256): partial [F/256][M][256] fp32 =
// relu(x . W1c^T + b1c) . W2c^T per 256-wide hidden chunk c; spe_launch_ffn_reduce_ln finishes.
// w1: W1 [F][256] fragment-packed; w2: chunk c's columns of W2 [256][F] packed at c * 256 * 256.
struct DecFfnArgs {
  const void* x; int ldx; int M, F;
  const void* w1; const float* b1; const void* w2;
  float* partial;
};
int spe_launch_decffn(const DecFfnArgs& a, hipStream_t s);
// y [M][ldy] = x . W^T (+ bias) + R[m % period] (decsa.hip; bf16, K = 256, N % 256 == 0; W packed)
struct DecQArgs {
  const void* x; int ldx; int M, N;
  const void* w; const float* bias;
  const void* R; int ldr; int period;   // optional row-periodic residual, bf16
  void* y; int ldy;
};
int spe_launch_decq(const DecQArgs& a, hipStream_t s);
// bf16 rows W [N][ld] (K = 256, N % 16 == 0) -> the fragment-packed layout above
int spe_launch_wfrag_pack(const void* w, int ld, int N, void* dst, hipStream_t s);
int spe_launch_decproj(const DecProjArgs& a, hipStream_t s);   // 1 = not applicable

// Fused FFN + residual + LayerNorm (bf16 only): y = LN(x + W2 relu(W1 x + b1) + b2).
// x / y may alias (each block reads and writes only its own rows).
struct FfnArgs {
  const void* x; int ldx;          // [M][256] bf16 (input and residual)
  const void* w1; int ld1;         // [F][ld1] bf16 (linear1.weight, K padded)
  const float* b1;                 // [F]
  const void* w2; int ld2;         // [256][ld2] bf16 (linear2.weight)
  const float* b2;                 // [256]
  const float* gamma; const float* beta;   // LayerNorm affine [256]
  void* y; int ldy;                // [M][256] bf16
  int M, D, F;
  const void* pos; void* ypos;     // optional: ypos = y + pos[m % pos_period] (bf16 [M][256])
  int pos_period;
  int splits; float* partial;      // optional split over F for few rows: fp32 [splits][M][256] workspace
  int row0;                        // first row of this launch's tiles (internal: the FFN tail launch)
  int w2_chunked;                  // w2 stored chunk-packed [F/32][256][32] (spe_launch_ffn_w2_chunk_pack); ld2 unused
  // pre-norm form (spe_launch_ffn_pre): n = LN(x; gamma, beta) on chip, y = x + W2 relu(W1 n + b1) + b2, and
  // beside it y2 = LN(y; gamma2, beta2) [M][ldy] bf16 (null: not stored); ypos = y2 + pos
  int pre;
  const float* gamma2; const float* beta2;
  void* y2;
};
// W2 [256][ld2] bf16 -> [F/32][256][32]: each 32-unit hidden chunk's columns as one contiguous block
int spe_launch_ffn_w2_chunk_pack(const void* w2, int ld2, int F, void* dst, hipStream_t s);
int spe_launch_ffn_ln(const FfnArgs& a, hipStream_t s);
int spe_launch_ffn_pre(const FfnArgs& a, hipStream_t s);
// y = LN(x + sum_s partial[s] + b2) over a.splits fp32 partials [splits][M][256] (ffn.hip)
int spe_launch_ffn_reduce_ln(const FfnArgs& a, hipStream_t s);
// fp32h3 encoder FFN + residual + LayerNorm in one pass (ffn_h3.hip): fp32 x / y [M][256], W1 as its
// h3 finalize planes fp16 [2][F][ld1] (rows scaled by 2^e1), meta1 [F/32][64] = (2^-e1, b1) of each
// 32-unit hidden chunk, W2 as fp16 planes [2][256][ld2] (rows scaled by 2^e2) with the columns of
// every 32-wide chunk in spe_ffn_h3_perm order, sinv2 = 2^-e2; amax_x = the bound on |x| (the A
// scale), sh = the power-of-two scale of the hidden activation (from its static bound)
struct FfnH3Args {
  const float* x; int ldx;
  float* y; int ldy;
  int M, D, F;
  const void* w1; int ld1; const float* meta1;
  const void* w2; int ld2; const float* sinv2; const float* b2;
  const float* gamma; const float* beta;
  const float* amax_x; float sh;
};
int spe_launch_ffn_h3(const FfnH3Args& a, hipStream_t s);
int spe_ffn_h3_perm(int p);
int spe_ffn_splits(int M, int F);  // split count spe_launch_ffn_ln would use for M rows (1 = none)

int spe_launch_preprocess(const uint8_t* frames, int B, int H, int W, int C, const double* bbox, int S,
                          float* images, float* clip_bbox, int32_t* status, hipStream_t s);
// SpeedSubmission's pad-to-square crop (REV/datasets/speed.py:92-160); images / crops_u8 nullable, not both
int spe_launch_preprocess_submission(const uint8_t* frames, int B, int H, int W, int C, const double* bbox, int S,
                                     float* images, uint8_t* crops_u8, float* clip_bbox, int32_t* status,
                                     hipStream_t s);
// The model input: the ImageNet-normalised fp32 batch [B][3][S][S] (f32), or the 8-bit crops
// [B][S][S][ch] (u8, ch = 1 grayscale -- SPEED's frames, Image.convert('RGB') replicating them --
// or 3 RGB) that to_tensor + Normalize (REV/datasets/speed.py:25-41) turn into it: the pack kernels
// normalise u8 / 255, (x - mean) / std in fp32, the reference's operation order (bit-identical to
// the f32 input computed the same way)
struct ImageSrc {
  const float* f32; const uint8_t* u8; int ch;
};
// amax (fp32 output only, nullable): max |image| atomically maxed in (the stem GEMM's fp32h3 scale input)
// cpad: channels per packed pixel (8; fp32 models' DETR stem: 4, one 16-byte chunk)
int spe_launch_pack_input(const ImageSrc& img, void* out, int B, int S, int dtype, hipStream_t s, float* amax = nullptr,
                          int cpad = 8);
inline int spe_launch_pack_input(const float* img, void* out, int B, int S, int dtype, hipStream_t s,
                                 float* amax = nullptr, int cpad = 8) {
  return spe_launch_pack_input(ImageSrc{img, nullptr, 0}, out, B, S, dtype, s, amax, cpad);
}
// bf16 [B][S+6][S+6][4], zero border of 3 (the pair-packed stem's input, forward.cpp)
int spe_launch_pack_input_pad4(const ImageSrc& img, void* out, int B, int S, hipStream_t s);
// bf16 pair-packed stem (x: spe_launch_pack_input_pad4 layout, w: [64][ldw] k = (kh*8 + kw)*4 + ci)
// + bias + ReLU + 3x3/s2/p1 max-pool in one pass (stempool.hip); out [B][Po][Po] rows of stride
// ldo.  Returns 1 when the shape does not fit the kernel.
bool spe_stempool_enabled();
bool spe_stempool_fits(int S);
int spe_launch_stempool(const void* x, const void* w, int ldw, const float* bias, void* out, int ldo, int B, int S,
                        hipStream_t s);
int spe_launch_maxpool3s2(const void* in, void* out, int B, int H, int W, int C, int Ho, int Wo,
                          int dtype, hipStream_t s, int ldo = 0);   // ldo: output row stride (0 = C)
int spe_launch_upsample2x(const void* in, void* out, int B, int H, int W, int C, int dtype, hipStream_t s);
// conv3x3(pad 1)(upsample2x(x)) from the per-tap low-resolution products z [B*H*W][9*C]
// (elementwise.hip); out rows of stride ldo (a channel slice of a concat buffer)
int spe_launch_upconv_combine(const void* z, void* out, int ldo, int B, int H, int W, int C, int dtype, hipStream_t s);
int spe_launch_layernorm(const void* x, const float* gamma, const float* beta, void* out, float* out_f32,
                         int M, int D, int dtype, hipStream_t s);

// GroupNorm(32, C), eps 1e-5, over NHWC rows [B*H*W][ld] (groupnorm.hip): y = (x - mean) rstd gamma[c] + beta[c]
// (+ res) (ReLU), mean / biased variance per (image, group).  Two launches: spe_launch_gn_stats writes Welford
// triples part[B][tiles][32][3] (spe_gn_scratch_bytes), spe_launch_gn_apply merges them and normalises; x, res and
// y may alias.  C / 32 in {2, 4, 8, 16, 32}, every ld >= C and a multiple of 8, pointers 16-byte aligned:
// spe_gn_check names the first violation (null = served), the launchers return -1 for one.
struct GroupNormArgs {
  const void* x; int ldx;
  const void* res; int ldr;        // residual added before the ReLU, or null
  const float* gamma; const float* beta;
  void* y; int ldy;
  int B, H, W, C, relu;
  float* part;
};
int spe_gn_tiles(int H, int W, int C);                     // partial-statistics tiles per image (dtype-independent)
int64_t spe_gn_scratch_bytes(int B, int H, int W, int C);
const char* spe_gn_check(const GroupNormArgs& a, int dtype);
int spe_launch_gn_stats(const GroupNormArgs& a, int dtype, hipStream_t s);
int spe_launch_gn_apply(const GroupNormArgs& a, int dtype, hipStream_t s);

struct HeadArgs {
  const float* hs;                 // [B*Q][256] fp32 (decoder_norm output of the last layer)
  int B, Q, D;
  const float* cls_wt; const float* cls_b;        // [D][12], [12]
  const float* pt_w0t; const float* pt_b0;        // [D][D]
  const float* pt_w1t; const float* pt_b1;
  const float* pt_w2t; const float* pt_b2;        // [D][2]
  const float* sg_w0t; const float* sg_b0;        // sigma head (nullable)
  const float* sg_w1t; const float* sg_b1;
  const float* sg_w2t; const float* sg_b2;        // [D][1]
  const float* clip_bbox;          // [B][4] (nullable -> no pixel rescale)
  float* logits;                   // [B][Q][12]
  float* points;                   // [B][Q][2] crop-normalised (sigmoid)
  float* probs;                    // [B][Q][12] softmax (nullable)
  float* points_px;                // [B][Q][2] image px (nullable)
  float* log_sigmas;               // [B][Q][2] (nullable)
  float* sigmas;                   // [B][Q][2] exp (nullable)
};
int spe_launch_heads(const HeadArgs& a, hipStream_t s);

// Set criterion (criterion.hip): Hungarian matching + losses for L layers of B images.
struct CritArgs {
  const float* logits;             // [L][B][Q][C]
  const float* points;             // [L][B][Q][2]
  const int32_t* tgt_labels;       // [B][T]
  const float* tgt_points;         // [B][T][2]
  int L, B, Q, C, T;
  float cost_class, cost_pts, eos_coef;
  double num_points;               // loss_points normaliser
  int32_t* match;                  // [L][B][T] matched query per target (out)
  double* partial;                 // [L][B][5] scratch
  double* losses;                  // [L][4] loss_ce, class_error, cardinality_error, loss_points (out)
};
int spe_launch_criterion(const CritArgs& a, hipStream_t s);

// UNC RT-DETR set criterion (criterion_sigma.hip): sigmoid / softmax matching cost, the L1 and the
// uncertainty point loss for L layers of B images.
struct CritSigmaArgs {
  const float* logits;             // [L][B][Q][C]
  const float* points;             // [L][B][Q][2]
  const float* log_sigmas;         // [L][B][Q][2], null when no layer has a sigma
  const int32_t* layer_has_sigma;  // [L] device flags: 0 -> the layer scores with s = 0
  const int32_t* tgt_labels;       // [B][T]
  const float* tgt_points;         // [B][T][2]
  int L, B, Q, C, T;
  float cost_class, cost_bbox;
  int sigmoid_cost;                // matching cost on sigmoid(logit) instead of softmax(logits)
  float eos_coef;
  double num_boxes;                // loss_bbox normaliser
  int32_t* match;                  // [L][B][T] matched query per target (out)
  double* partial;                 // spe_criterion_sigma_partial_bytes(L, B) of scratch
  double* losses;                  // [L][6] loss_ce, class_error, cardinality_error, loss_bbox (points),
                                   // loss_bbox (points_uncert), points_different (out)
};
size_t spe_criterion_sigma_partial_bytes(int L, int B);
int spe_launch_criterion_sigma(const CritSigmaArgs& a, hipStream_t s);

// Multi-model keypoint fusion (ensemble.hip): M models' PostProcess outputs -> one fused
// keypoint set per image in spe_pnp_batch's input layout.
struct EnsembleArgs {
  const float* points;             // [M][B][Q][2] image px
  const float* probs;              // [M][B][Q][C]
  int M, B, Q, C;
  float* fused_points;             // [B][C-1][2]
  float* fused_probs;              // [B][C-1][C] one-hot rows (background padding)
};
int spe_launch_ensemble_fuse(const EnsembleArgs& a, hipStream_t s);
// The sigma-weighted fusion (include/spe.h spe_ensemble_fuse_sigma): one measurement per model and
// label, gated inverse-variance mean, fused sigma; the same output layout plus sigmas and counts.
struct EnsembleSigmaArgs {
  const float* points;             // [M][B][Q][2] image px
  const float* probs;              // [M][B][Q][C]
  const float* sigmas;             // [M][B][Q][2] in the model's unit
  const float* sigma_scale;        // [B][2] px per sigma unit, or nullptr (1)
  int M, B, Q, C;
  float sigma_floor, gate;
  float* fused_points;             // [B][C-1][2]
  float* fused_probs;              // [B][C-1][C] fused score in the label's column (background padding)
  float* fused_sigmas;             // [B][C-1][2] in the input's unit
  int32_t* n_pooled;               // [B][C-1]
  int32_t* n_kept;                 // [B][C-1]
};
int spe_launch_ensemble_fuse_sigma(const EnsembleSigmaArgs& a, hipStream_t s);
// Lens distortion in front of the solvers (lens.hip; include/spe.h spe_undistort_points /
// spe_distort_points): one thread per point, n = B * Q points, every array 8-byte aligned.
struct LensArgs {
  const float* points;             // [n][2] px (undistort: distorted, distort: ideal)
  const float* sigmas;             // [n][2] in the caller's unit, or nullptr
  const float* sigma_scale;        // [B][2] px per sigma unit, or nullptr (1)
  size_t n;
  int Q;
  const double* K;                 // 3x3 row-major
  const double* dist;              // k1, k2, p1, p2, k3
  int iters;
  float* points_out;               // [n][2] px; may be `points`
  float* sigmas_out;               // [n][2] or nullptr; may be `sigmas`
  uint8_t* status;                 // [n] or nullptr
};
int spe_launch_undistort_points(const LensArgs& a, hipStream_t s);
int spe_launch_distort_points(const LensArgs& a, hipStream_t s);
int spe_launch_postprocess(const float* logits, const float* points, const float* clip_bbox, int B, int Q,
                           float* probs, float* points_px, hipStream_t s);

// ---- UNC RT-DETR (rtdetr.hip; rtdetr_model.cpp and, for the backbone kernels below, its rtdetr_<family>.cpp files)
// nearest x2 (mode 0) / bicubic x0.5 (mode 1) resample of NHWC [B][H][W][C] (row stride ldi)
// into [B][Ho][Wo] rows of stride ldo (a channel slice of a concat buffer)
int spe_launch_resample2x(const void* in, int ldi, void* out, int ldo, int B, int H, int W, int C, int mode, int dtype,
                          hipStream_t s);
struct RtSelectArgs {
  const float* logits; int C;      // enc_score_head [level-major rows][C] fp32
  const void* memory; int ldm;     // output_memory (enc_output), level-major rows, T
  const float* anchors;            // [L][2] per-image token anchors (logit domain)
  int B, Q, D, levels;
  int lvl_start[5];                // token offsets of the levels within an image, [levels] = L
  int* topk;                       // [B][Q] selected token indices, descending score
  void* target; int ldt;           // [B*Q][D] T gathered output_memory rows
  float* sel_logits;               // [B*Q][C]
  float* sel_anchors;              // [B*Q][2]
};
int spe_launch_query_select(const RtSelectArgs& a, int dtype, hipStream_t s);
int spe_launch_qpos_hidden(const float* ref, const float* w0, const float* b0, void* out, int rows, int H, int dtype,
                           hipStream_t s);
struct RtDeformArgs {
  const void* value; int ldv;      // level-major rows [lvl_rows0[l] + b*H_l*W_l + y*W_l + x], T, heads h*32+c
  const float* so_aw; int ld_so;   // [rows][2*H*NL*NP offsets | H*NL*NP attention logits] fp32
  const float* ref;                // [rows][2] reference points (sigmoid domain)
  void* out; int ldo;              // [rows][256] T
  int rows, Q, heads, levels, points;
  int lvl_h[4], lvl_w[4], lvl_rows0[4];
};
int spe_launch_msdeform(const RtDeformArgs& a, int dtype, hipStream_t s);
// The head-averaged map of one msdeform call (the diagnostic tap of spe_rtdetr_forward_attention): the weight
// every memory token of the row's image receives through the bilinear corners of the 8 x levels x points
// samples.  Reads what msdeform reads but the value, so one kernel serves both model dtypes.
struct RtDeformMapArgs {
  const float* so_aw; int ld_so;   // as RtDeformArgs
  const float* ref;                // [rows][2]
  float* map;                      // [rows][L] token order of one image: level-major, y * W_l + x (nullable)
  float* loc;                      // [rows][H][NL][NP][2] normalised sampling locations (x, y) (nullable)
  float* weights;                  // [rows][H][NL][NP] softmaxed attention weights (nullable)
  int rows, Q, heads, levels, points;
  int lvl_h[4], lvl_w[4];
  int lvl_start[5];                // per-image token offsets, [levels] = L <= 12288
};
int spe_launch_deform_map(const RtDeformMapArgs& a, hipStream_t s);   // -5: arguments outside the contract
struct RtHeadArgs {
  int rows, Q, C;
  const float* hs;                 // [rows][256] fp32 layer output (score head input; null: no score head)
  const float* cls_w; const float* cls_b;   // [C][256], [C]
  const void* h2; int ld_h2;       // T: box hidden (cols 0..255), sigma hidden (cols 256..511)
  const float* box_w2; const float* box_b2; // [2][256], [2]
  const float* sig_w2; const float* sig_b2; // [1][256], [1] (null: no sigma head)
  const float* pt_add; int pt_add_invsig;   // [rows][2]: anchors, or reference points (inverse_sigmoid)
  float* logits; float* probs;     // [rows][C]
  float* points;                   // [rows][2] sigmoid
  const float* clip_bbox; float* points_px;
  float* log_sigmas; float* sigmas;         // [rows][2]
};
int spe_launch_head_finish(const RtHeadArgs& a, int dtype, hipStream_t s);

// ---- MobileNetV3_Large backbone kernels (mbv3.hip).  Every launcher returns -1 before any launch
// when the shapes are outside its contract, 0 or a hipError_t otherwise.
enum { MB_ACT_NONE = 0, MB_ACT_RELU = 1, MB_ACT_HSWISH = 4 };   // Hardswish: x relu6(x + 3) / 6
// conv1 3x3/s2/p1 3 -> 16 + bias + Hardswish from the fp32 NCHW batch [B][3][S][S] (S even) into NHWC T
// [B][S/2][S/2][16]; w fp32 [27][16] with k = (ci*3 + kh)*3 + kw.  A u8 source ([B][S][S][ch] crops, ch 1 / 3,
// 4-byte aligned, S % 32 == 0, B <= 65535) takes the tiled 8-bit kernel (stem_u8.h), bit-identical to the fp32
// kernel on the batch normalised from the crops.
int spe_launch_mb_stem(const ImageSrc& src, const float* w, const float* bias, void* out, int B, int S, int dtype,
                       hipStream_t s);
// depthwise k x k, pad k/2, over NHWC T.  Contract: k 3 or 5; stride 1, or 2 with even H and W (Ho = H /
// stride); C % 8 == 0; B <= 65535.  w fp32 [k*k][C] (BatchNorm scale folded in), bias fp32 [C].
// pool (nullable): fp32 [B][spe_mb_dwconv_tiles(Ho, Wo)][C], per 8 x 8 output tile the sum of the
// stored outputs, reduced in a fixed order (two runs give the same bits).
struct MbDwArgs {
  const void* in; void* out;
  const float* w; const float* bias;
  float* pool;
  int B, H, W, C, k, stride, act;
  int Ho, Wo, cg;                  // set by the launcher
};
int spe_mb_dwconv_tiles(int Ho, int Wo);
bool spe_mb_dwconv_fits(int B, int H, int W, int C, int k, int stride);
int spe_launch_mb_dwconv(MbDwArgs a, int dtype, hipStream_t s);
// SE gate: scale[b][c] = hardsigmoid(w2 . relu(w1 . mean_b + b1)) with mean_b[c] = inv_hw * sum over tiles
// of pool[b][t][c]; w1 fp32 [hidden][C] (BatchNorm folded), b1 [hidden], w2t fp32 [hidden][C] (the second
// conv's weight transposed).  C <= 1024, hidden <= 256.  fp32 throughout in both model dtypes.
// b2 (nullable, last so that older initialisers leave it null): fp32 [C], the second conv's bias (GhostNetV2).
struct MbSeArgs {
  const float* pool; int tiles; float inv_hw;
  const float* w1; const float* b1; const float* w2t;
  float* scale;
  int B, C, hidden;
  const float* b2;
};
int spe_launch_mb_se_gate(const MbSeArgs& a, hipStream_t s);
// C[m][n] = act((A . scale) . W^T + bias + R): A row m = output pixel (b, oy, ox) of an NHWC T tensor
// [*][H][W][lda >= Cin], column k = (kh*KW + kw)*Cin + ci (zero outside the image); W T [N][ldb]; bias
// fp32 [N] (nullable); scale fp32 [B][K] (nullable, 1x1 only): A[m][k] * scale[b][k], rounded to T;
// R T [M][ldr] (nullable), added before the activation.  Contract: N, K, Cin, lda, ldb, ldc, ldr % 8 ==
// 0; M = B * Ho * Wo.
struct MbGemmArgs {
  const void* A; int lda;
  const void* Bw; int ldb;
  const float* bias; const float* scale;
  const void* R; int ldr;
  void* C; int ldc;
  int M, N, K;
  int H, W, Cin, KH, KW, stride, pad, Ho, Wo;
  int act;
};
bool spe_mb_gemm_fits(const MbGemmArgs& g);
int spe_launch_mb_gemm(const MbGemmArgs& g, int dtype, hipStream_t s);
// MobileNetV3_Small entry (mbv3s.hip): image -> pooled / skip / t2, NHWC T [B][S/4][S/4][16] each, and t2's SE
// pool partials fp32 [B][spe_mbs_entry_tiles(S)][16] (nullable; mb_dwconv's layout and fixed-order reduction).
// w: fp32 [MBS_W_FLOATS], BatchNorm folded: conv1 [27][16] (k = (ci*3 + kh)*3 + kw) + bias, block 0's expand
// [ci][co] + bias, its depthwise [9][16] + bias, its skip depthwise [9][16] + bias.  Contract: S % 16 == 0,
// 32 <= S <= 4096, B <= 65535; a u8 source has ch 1 or 3 (no alignment demand: the patch is read by bytes).
enum {
  MBS_W_STEM = 0, MBS_W_STEM_B = 432, MBS_W_EXP = 448, MBS_W_EXP_B = 704, MBS_W_DW = 720, MBS_W_DW_B = 864,
  MBS_W_SKIP = 880, MBS_W_SKIP_B = 1024, MBS_W_FLOATS = 1040
};
struct MbsEntryArgs {
  ImageSrc src;
  const float* w;
  void* pooled; void* skip; void* t2;
  float* pool;
  int B, S;
};
bool spe_mbs_entry_enabled();                     // SPE_MBS_ENTRY (default 1): 0 = block 0 launch by launch
bool spe_mbs_entry_fits(int B, int S);
int spe_mbs_entry_tiles(int S);
int spe_launch_mbs_entry(const MbsEntryArgs& a, int dtype, hipStream_t s);
// NHWC T [B][HW][C] -> NCHW fp32
int spe_launch_mb_to_nchw(const void* in, float* out, int B, int HW, int C, int dtype, hipStream_t s);

// ---- GhostNetV2 backbone kernels (ghostv2.hip).  Every launcher returns -1 before any launch when the
// shapes are outside its contract, 0 or a hipError_t otherwise.
enum { GH_POST_NONE = 0, GH_POST_GATE = 1, GH_POST_RESIDUAL = 2 };
// conv_stem 3x3/s2/p1 3 -> 16 from the fp32 NCHW batch [B][3][S][S] (S even) into two NHWC T tensors
// [B][S/2][S/2][16]: raw = the conv output, act = relu(raw * scale + shift) (bn1 folded); w fp32 [27][16].
// A u8 source: as spe_launch_mb_stem's.
int spe_launch_gh_stem(const ImageSrc& src, const float* w, const float* scale, const float* shift, void* raw, void* act,
                       int B, int S, int dtype, hipStream_t s);
// Ghost module tail.  x1: NHWC T, pixel stride ldx, channels [xoff, xoff + half); x2 = act(dw3x3(x1) + bias),
// w fp32 [9][half] (BatchNorm folded), act none / ReLU.  out T [B][H][W][2 half]: out[:half] = post(x1),
// out[half:] = post(x2); post GATE: * gate[b][h/2][w/2][c] (T [B][H/2][W/2][2 half], H and W even), post
// RESIDUAL: + resid[b][h][w][c] (T, out's layout).  pool (nullable): fp32 [B][spe_gh_cheap_tiles(H, W)][2 half],
// per 8 x 8 tile the sum of the stored outputs in a fixed order.  Contract: half, ldx, xoff % 8 == 0,
// ldx >= xoff + half, B <= 65535.  out must not alias x1.
struct GhCheapArgs {
  const void* x1; int ldx, xoff;
  const float* w; const float* bias;
  void* out;
  const void* gate; const void* resid;
  float* pool;
  int B, H, W, half, act, post;
  int cg;                          // set by the launcher
};
int spe_gh_cheap_tiles(int H, int W);
bool spe_gh_cheap_fits(const GhCheapArgs& a);
int spe_launch_gh_cheap(GhCheapArgs a, int dtype, hipStream_t s);
// DFC gate: gate = sigmoid(dw5x1(dw1x5(x) + b1) + b2) over NHWC T [B][H][W][C], H, W <= 32, C % 8 == 0;
// w1 / w2 fp32 [5][C] (tap-major, BatchNorm folded), b1 / b2 fp32 [C]; zero padding on both convs' inputs
struct GhDfcArgs {
  const void* x; void* gate;
  const float* w1; const float* b1; const float* w2; const float* b2;
  int B, H, W, C;
  int cg;                          // set by the launcher
};
bool spe_gh_dfc_fits(int B, int H, int W, int C);
int spe_launch_gh_dfc(GhDfcArgs a, int dtype, hipStream_t s);
// 2x2 mean, NHWC T [B][H][W][C] -> [B][H/2][W/2][C]; H, W even, C % 8 == 0
bool spe_gh_pool2_fits(int B, int H, int W, int C);
int spe_launch_gh_pool2(const void* in, void* out, int B, int H, int W, int C, int dtype, hipStream_t s);
