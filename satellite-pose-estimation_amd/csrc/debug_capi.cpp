// Kernel-level test hooks (declared in include/spe.h, "kernel test hooks"): thin C entry points
// that launch one kernel family on caller-provided device buffers, so tests/ can check each
// kernel against a plain torch reference of the same op at awkward shapes (edges, ragged
// tiles, strides) — the forward pass alone would hide a wrong-but-normalised intermediate.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/spe.h"
#include "model_state.h"

namespace {
thread_local const void* g_planes = nullptr;   // spe_debug_gemm_planes -> spe_debug_gemm
thread_local int g_plane_rows = 0;
}  // namespace

extern "C" {

int spe_debug_gemm(void* stream, int dtype, int mode, const void* A, int lda, const void* P, int ldp, int prow,
                   int H, int W, int Cin, int KH, int KW, int stride, int pad, const void* Bw, int ldb, int M, int N,
                   int K, const float* bias, const void* R, int ldr, int act_code, void* C, int ldc, int out_f32, int vt_T,
                   int vt_B, int r_period, const float* ln_g, const float* ln_b, int out_f16) {
  GemmArgs g{};
  g.A = A; g.lda = lda; g.P = P; g.ldp = ldp; g.prow = prow;
  g.H = H; g.W = W; g.Cin = Cin; g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad;
  g.Ho = mode == GEMM_CONV ? (H + 2 * pad - KH) / stride + 1 : 0;
  g.Wo = mode == GEMM_CONV ? (W + 2 * pad - KW) / stride + 1 : 0;
  g.B = Bw; g.ldb = ldb; g.M = M; g.N = N; g.K = K;
  g.bias = bias; g.R = R; g.ldr = ldr; g.act = act_code & 255; g.res_post = (act_code >> 8) & 1; g.C = C; g.ldc = ldc; g.out_f32 = out_f32;
  g.vt_swz = (act_code >> 9) & 1;
  g.vt_T = vt_T; g.vt_B = vt_B;
  g.r_period = r_period;
  g.ln_g = ln_g; g.ln_b = ln_b;
  g.out_f16 = out_f16;
  g.B6 = g_planes;
  g.b6_rows = g_plane_rows;
  int rc = spe_launch_gemm(g, dtype, mode, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_LAUNCH, "gemm launch rejected its arguments") : rc;
}

int spe_debug_gemm_planes(void* stream, int dtype, int mode, const void* A, int lda, const void* P, int ldp, int prow,
                          int H, int W, int Cin, int KH, int KW, int stride, int pad, const void* Bw, int ldb, int M,
                          int N, int K, const float* bias, const void* R, int ldr, int act_code, void* C, int ldc,
                          const void* planes, int plane_rows) {
  g_planes = planes;
  g_plane_rows = plane_rows;
  const int rc = spe_debug_gemm(stream, dtype, mode, A, lda, P, ldp, prow, H, W, Cin, KH, KW, stride, pad, Bw, ldb, M, N,
                                K, bias, R, ldr, act_code, C, ldc, 0, 0, 0, 0, nullptr, nullptr, 0);
  g_planes = nullptr;
  g_plane_rows = 0;
  return rc;
}

int spe_debug_gemm_h3(void* stream, int mode, const void* A, int lda, int H, int W, int Cin, int KH, int KW, int stride,
                      int pad, int ldb, int M, int N, int K, const float* bias, const void* R, int ldr, int act_code,
                      void* C, int ldc, const void* planes, int plane_rows, const float* sinv, const float* amax_a,
                      float* amax_c, float amax_c_mul) {
  if (!A || !C || !planes || !sinv || M < 0 || N <= 0 || K <= 0) return spe_fail(SPE_E_ARG, "bad argument");
  GemmArgs g{};
  g.A = A; g.lda = lda;
  g.H = H; g.W = W; g.Cin = Cin; g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad;
  g.Ho = mode == GEMM_CONV ? (H + 2 * pad - KH) / stride + 1 : 0;
  g.Wo = mode == GEMM_CONV ? (W + 2 * pad - KW) / stride + 1 : 0;
  g.B = planes; g.ldb = ldb; g.M = M; g.N = N; g.K = K;
  g.bias = bias; g.R = R; g.ldr = ldr; g.act = act_code & 255; g.C = C; g.ldc = ldc;
  g.H3 = planes; g.h3_rows = plane_rows; g.h3_sinv = sinv; g.amax_a = amax_a; g.amax_c = amax_c;
  g.amax_c_mul = amax_c_mul;
  // (the h3 kernels only: through spe_launch_gemm an unserved shape would run the x6 kernel, which
  // reads the fp16 planes as fp32 weights)
  const int rc = spe_launch_gemm_h3(g, mode, (hipStream_t)stream);
  if (rc == 1) return spe_fail(SPE_E_LAUNCH, "shape not served by the fp32h3 kernel");
  return rc < 0 ? spe_fail(SPE_E_LAUNCH, "gemm launch rejected its arguments") : rc;
}

int spe_debug_gemm_path(void) { return spe_gemm_last_path; }

int spe_debug_ffn_h3(void* stream, const float* x, int ldx, float* y, int ldy, int M, int F, const void* w1, int ld1,
                     const float* meta1, const void* w2, int ld2, const float* sinv2, const float* b2,
                     const float* gamma, const float* beta, const float* amax_x, float sh) {
  FfnH3Args a{};
  a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.M = M; a.D = 256; a.F = F;
  a.w1 = w1; a.ld1 = ld1; a.meta1 = meta1; a.w2 = w2; a.ld2 = ld2; a.sinv2 = sinv2; a.b2 = b2;
  a.gamma = gamma; a.beta = beta; a.amax_x = amax_x; a.sh = sh;
  const int rc = spe_launch_ffn_h3(a, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_ARG, "ffn_h3 launch rejected its arguments") : rc;
}

int spe_debug_ffn_h3_perm(int p) { return p >= 0 && p < 32 ? spe_ffn_h3_perm(p) : -1; }

int spe_debug_attention(void* stream, int dtype, const void* q, int ldq, const void* k, int ldk, const void* vt,
                        void* o, int ldo, int B, int H, int Tq, int Tk, float scale) {
  AttnArgs a{};
  a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldk; a.vt = vt; a.o = o; a.ldo = ldo;
  a.B = B; a.H = H; a.Tq = Tq; a.Tk = Tk; a.scale = scale;
  a.vt_swz = (dtype >> 8) & 1;
  a.presplit = (dtype >> 9) & 1;
  a.v_f16 = (dtype >> 10) & 1;                     // (unscaled fp16 V^T planes: v_amax null)
  int rc = spe_launch_attention(a, dtype & 255, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_LAUNCH, "attention launch rejected its arguments") : rc;
}

int spe_debug_attn_map(void* stream, const void* q, const void* k, int B, int H, int Tq, int Tk, int dtype, float* out) {
  if (!q || !k || !out || B <= 0 || H != 8 || Tq <= 0 || Tk <= 0) return spe_fail(SPE_E_ARG, "bad argument");
  const int dt = dtype & 255;
  if (dt != SPE_DTYPE_BF16 && dt != SPE_DTYPE_F32 && dt != SPE_DTYPE_F16) return spe_fail(SPE_E_ARG, "attn_map: dtype bf16, fp16 or fp32");
  AttnMapArgs a{};
  a.q = q; a.k = k; a.out = out;
  a.B = B; a.H = H; a.Tq = Tq; a.Tk = Tk;
  if (dtype & 0x100) {                           // the folded decoder form: q' [B][Tq][8*256], k [B][Tk][256]
    if (dt != SPE_DTYPE_BF16) return spe_fail(SPE_E_ARG, "attn_map: the folded form is bf16");
    a.q_sb = (long long)Tq * H * 256; a.q_sh = 256; a.ldq = H * 256;
    a.k_sb = (long long)Tk * 256; a.k_sh = 0; a.ldk = 256;
    a.head_dim = 256; a.base2 = 1; a.scale = 1.f;
  } else {                                       // q [B][H][Tq][32], k [B][H][Tk][32]
    a.q_sb = (long long)H * Tq * 32; a.q_sh = (long long)Tq * 32; a.ldq = 32;
    a.k_sb = (long long)H * Tk * 32; a.k_sh = (long long)Tk * 32; a.ldk = 32;
    a.head_dim = 32; a.scale = 1.0f / std::sqrt(32.0f);   // (forward.cpp's)
  }
  const int rc = spe_launch_attn_map(a, dt, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_LAUNCH, "attn_map launch rejected its arguments") : rc;
}

int spe_debug_layernorm(void* stream, int dtype, const void* x, const float* gamma, const float* beta, void* out,
                        float* out_f32, int M, int D) {
  int rc = spe_launch_layernorm(x, gamma, beta, out, out_f32, M, D, dtype, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_LAUNCH, "layernorm launch rejected its arguments") : rc;
}

int spe_debug_groupnorm(void* stream, int dtype, const void* x, int ldx, const void* residual, int ldr,
                        const float* gamma, const float* beta, void* y, int ldy, int B, int H, int W, int C, int relu,
                        void* scratch, int64_t scratch_bytes) {
  GroupNormArgs a{};
  a.x = x; a.ldx = ldx; a.res = residual; a.ldr = ldr; a.gamma = gamma; a.beta = beta; a.y = y; a.ldy = ldy;
  a.B = B; a.H = H; a.W = W; a.C = C; a.relu = relu; a.part = (float*)scratch;
  const int dt = dtype == SPE_DTYPE_BF16_ ? (int)SPE_DTYPE_BF16 : dtype == SPE_DTYPE_F32_ ? (int)SPE_DTYPE_F32 : -1;
  if (const char* why = spe_gn_check(a, dt)) return spe_fail(SPE_E_ARG, why);
  if (scratch_bytes < spe_gn_scratch_bytes(B, H, W, C)) return spe_fail(SPE_E_ARG, "groupnorm: scratch below the stated size");
  int rc = spe_launch_gn_stats(a, dt, (hipStream_t)stream);
  if (rc == 0) rc = spe_launch_gn_apply(a, dt, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_LAUNCH, "groupnorm launch rejected its arguments") : rc;
}

int64_t spe_debug_groupnorm_scratch_bytes(int B, int H, int W, int C) {
  if (B <= 0 || C <= 0 || C % 32) return 0;
  return spe_gn_scratch_bytes(B, H, W, C);
}

int spe_debug_ffn_pre(void* stream, const void* x, int ldx, const void* w1, int ld1, const float* b1, const void* w2,
                      int ld2, const float* b2, const float* gamma, const float* beta, void* y, int ldy, int M, int D,
                      int F, float* partial, int splits, const float* gamma2, const float* beta2, void* y2,
                      const void* pos, int pos_period, void* ypos) {
  FfnArgs a{};
  a.x = x; a.ldx = ldx; a.w1 = w1; a.ld1 = ld1; a.b1 = b1; a.w2 = w2; a.ld2 = ld2; a.b2 = b2;
  a.gamma = gamma; a.beta = beta; a.y = y; a.ldy = ldy; a.M = M; a.D = D; a.F = F;
  if (ld2 == 0) {                               // w2 chunk-packed [F/32][256][32]
    a.w2_chunked = 1;
    a.ld2 = F;
  }
  a.partial = partial; a.splits = splits;
  a.gamma2 = gamma2; a.beta2 = beta2; a.y2 = y2;
  a.pos = pos; a.pos_period = pos_period; a.ypos = ypos;
  const int rc = spe_launch_ffn_pre(a, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_ARG, "ffn_pre launch rejected its arguments") : rc;
}

int spe_debug_oproj_pre(void* stream, const void* A, int lda, const void* W, int ldb, const float* bias, const void* R,
                        int ldr, void* C, int ldc, int M) {
  GemmArgs g{};
  g.A = A; g.lda = lda; g.B = W; g.ldb = ldb; g.M = M; g.N = 256; g.K = 256;
  g.bias = bias; g.R = R; g.ldr = ldr; g.C = C; g.ldc = ldc;
  const int rc = spe_launch_lnproj_pre(g, (hipStream_t)stream);
  if (rc == 1) return spe_fail(SPE_E_LAUNCH, "shape not served by the pre-norm out-projection kernel");
  return rc < 0 ? spe_fail(SPE_E_LAUNCH, "oproj_pre launch rejected its arguments") : rc;
}

int spe_debug_ffn(void* stream, const void* x, int ldx, const void* w1, int ld1, const float* b1, const void* w2,
                  int ld2, const float* b2, const float* gamma, const float* beta, void* y, int ldy, int M, int D,
                  int F, float* partial, int splits) {
  FfnArgs a{};
  a.x = x; a.ldx = ldx; a.w1 = w1; a.ld1 = ld1; a.b1 = b1; a.w2 = w2; a.ld2 = ld2; a.b2 = b2;
  a.gamma = gamma; a.beta = beta; a.y = y; a.ldy = ldy; a.M = M; a.D = D; a.F = F;
  if (ld2 == 0) {                               // w2 chunk-packed [F/32][256][32] (the model's bf16 encoder form)
    a.w2_chunked = 1;
    a.ld2 = F;
  }
  a.partial = partial; a.splits = splits;
  int rc = spe_launch_ffn_ln(a, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_LAUNCH, "ffn launch rejected its arguments") : rc;
}

int spe_debug_upconv(void* stream, int dtype, const void* z, void* out, int ldo, int B, int H, int W, int C) {
  if (!z || !out || B < 0 || H < 1 || W < 1 || C < 1) return spe_fail(SPE_E_ARG, "bad argument");
  int rc = spe_launch_upconv_combine(z, out, ldo, B, H, W, C, dtype, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_LAUNCH, "upconv launch rejected its arguments") : rc;
}

int spe_debug_xattn(void* stream, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* u,
                    int ldu, const void* wv, const float* bv, void* o, int ldo, int B, int Q, int T, int splits,
                    float* partial_scratch) {
  XattnArgs a{};
  a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldk; a.v = v; a.ldv = ldv; a.u = u; a.ldu = ldu;
  a.wv = wv; a.bv = bv; a.o = o; a.ldo = ldo;
  a.B = B; a.Q = Q; a.T = T; a.splits = splits > 0 ? splits : spe_xattn_splits(B, Q, T);
  const size_t rows = (size_t)a.splits * B * 8 * Q;
  a.pm = partial_scratch; a.pl = partial_scratch ? partial_scratch + rows : nullptr;
  a.pu = partial_scratch ? partial_scratch + 2 * rows : nullptr;
  const int rc = spe_launch_xattn(a, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_LAUNCH, "xattn launch rejected its arguments") : rc;
}

int spe_debug_xattn_h3(void* stream, const float* q, int ldq, const float* mem, const float* pos, const float* mem_amax,
                       const float* wv, const float* bv, float* o, int ldo, float* o_amax, int B, int Q, int T,
                       int splits, float* partial_scratch, void* plane_scratch) {
  if (!q || !mem || !pos || !mem_amax || !wv || !bv || !o || !partial_scratch || !plane_scratch || B < 0 || Q < 1 ||
      T < 1)
    return spe_fail(SPE_E_ARG, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  char* kp = (char*)plane_scratch;
  char* vp = kp + (size_t)B * T * 1024;
  if (spe_launch_xattn_h3_split(mem, pos, mem_amax, kp, vp, B, T, s) != 0)
    return spe_fail(SPE_E_LAUNCH, "xattn_h3 split launch failed");
  XattnArgs a{};
  a.q = q; a.ldq = ldq; a.k = kp; a.ldk = 512; a.v = vp; a.ldv = 512;
  a.wv = wv; a.bv = bv; a.o = o; a.ldo = ldo;
  a.B = B; a.Q = Q; a.T = T; a.splits = splits > 0 ? splits : spe_xattn_splits(B, Q, T);
  const size_t rows = (size_t)a.splits * B * 8 * Q;
  a.pm = partial_scratch; a.pl = partial_scratch + rows; a.pu = partial_scratch + 2 * rows;
  a.mem_amax = mem_amax; a.o_amax = o_amax;
  const int rc = spe_launch_xattn_h3(a, s);
  return rc != 0 ? spe_fail(SPE_E_LAUNCH, "xattn_h3 launch rejected its arguments") : 0;
}

int spe_debug_btail(void* stream, const void* a, int lda, int k1, const void* r, const void* w3, int ld3,
                    const float* b3, void* y, const void* w1p, int ld1, const float* b1, void* z, int n2, int M) {
  if (!a || !w3 || !b3 || !y || !w1p || !b1 || !z || M < 0) return spe_fail(SPE_E_ARG, "bad argument");
  BtailArgs t{};
  t.A = a; t.lda = lda; t.k1 = k1; t.R = r; t.ldr = 256;
  t.w3 = w3; t.ld3 = ld3; t.b3 = b3; t.y = y; t.ldy = 256; t.n1 = 256;
  t.w1 = w1p; t.ld1 = ld1; t.b1 = b1; t.z = z; t.ldz = n2; t.n2 = n2; t.M = M;
  t.rows = spe_btail_rows_enabled();
  const int rc = spe_launch_btail(t, (hipStream_t)stream);
  return rc != 0 ? spe_fail(SPE_E_LAUNCH, "btail launch rejected its arguments") : 0;
}

// btail.hip with every stride, the row-piece form (rows: 0 = 8-byte, 1 = 16-byte pieces) and, with H > 0 and W > 0, the compact y store requested for
// M = B * H * W pixels.  0 = launched, y stored whole; 2 = launched, y stored as the even pixels
// [B][H/2][W/2][256] (row stride ldy); 1 = not served (nothing launched); < 0 = bad argument
int spe_debug_btail_rows(void* stream, const void* a, int lda, int k1, const void* r, int ldr, const void* w3, int ld3,
                         const float* b3, void* y, int ldy, const void* w1p, int ld1, const float* b1, void* z, int ldz,
                         int n2, int M, int rows, int H, int W) {
  if (!a || !w3 || !b3 || !y || !w1p || !b1 || !z || M < 0 || H < 0 || W < 0) return spe_fail(SPE_E_ARG, "bad argument");
  BtailArgs t{};
  t.A = a; t.lda = lda; t.k1 = k1; t.R = r; t.ldr = ldr;
  t.w3 = w3; t.ld3 = ld3; t.b3 = b3; t.y = y; t.ldy = ldy; t.n1 = 256;
  t.w1 = w1p; t.ld1 = ld1; t.b1 = b1; t.z = z; t.ldz = ldz; t.n2 = n2; t.M = M;
  t.rows = rows != 0; t.ycompact = H > 0 && W > 0; t.H = H; t.W = W;
  const int rc = spe_launch_btail(t, (hipStream_t)stream);
  if (rc != 0 && rc != 1) return spe_fail(SPE_E_LAUNCH, "btail launch failed");
  return rc == 0 && spe_btail_ycompact_serves(t) ? 2 : rc;
}

// 0 = launched, 1 = not served (nothing launched, y and z untouched), < 0 = bad argument
int spe_debug_btail_wide(void* stream, const void* a, int lda, int k1, const void* r, int ldr, const void* w3, int ld3,
                         const float* b3, void* y, int ldy, int n1, const void* w1p, int ld1, const float* b1, void* z,
                         int ldz, int n2, int M) {
  if (!a || !w3 || !b3 || !y || !w1p || !b1 || !z || M < 0) return spe_fail(SPE_E_ARG, "bad argument");
  BtailArgs t{};
  t.A = a; t.lda = lda; t.k1 = k1; t.R = r; t.ldr = ldr;
  t.w3 = w3; t.ld3 = ld3; t.b3 = b3; t.y = y; t.ldy = ldy; t.n1 = n1;
  t.w1 = w1p; t.ld1 = ld1; t.b1 = b1; t.z = z; t.ldz = ldz; t.n2 = n2; t.M = M;
  const int rc = spe_launch_btail_wide(t, (hipStream_t)stream);
  return rc != 0 && rc != 1 ? spe_fail(SPE_E_LAUNCH, "btail_wide launch failed") : rc;
}

int spe_debug_btail_wide_proj(void* stream, const void* a, int lda, int k1, const void* r, int ldr, const void* w3,
                              int ld3, const float* b3, void* y, int ldy, int n1, const void* w1p, int ld1,
                              const float* b1, void* z, int ldz, int n2, int M, int relu_z) {
  if (!a || !w3 || !b3 || !w1p || !b1 || !z || M < 0) return spe_fail(SPE_E_ARG, "bad argument");
  BtailArgs t{};
  t.A = a; t.lda = lda; t.k1 = k1; t.R = r; t.ldr = ldr;
  t.w3 = w3; t.ld3 = ld3; t.b3 = b3; t.y = y; t.ldy = ldy; t.n1 = n1;
  t.w1 = w1p; t.ld1 = ld1; t.b1 = b1; t.z = z; t.ldz = ldz; t.n2 = n2; t.M = M;
  const int rc = spe_launch_btail_wide_proj(t, relu_z != 0, (hipStream_t)stream);
  return rc != 0 && rc != 1 ? spe_fail(SPE_E_LAUNCH, "btail_wide_proj launch failed") : rc;
}

// The decoder kernels read fragment-packed weights (spe_launch_wfrag_pack).  The hooks take
// row-major rows (ld > 0) and pack them into scratch of their own, released after the launch has
// completed, or already-packed weights (ld == 0, spe_debug_wfrag_pack: timing loops).
namespace {
struct Frags {
  std::vector<void*> bufs;
  hipStream_t s;
  int err = 0;
  explicit Frags(hipStream_t st) : s(st) {}
  const void* get(const void* w, int ld, int N) {
    if (ld == 0 || !w) return w;
    void* p = nullptr;
    if (hipMalloc(&p, (size_t)N * 256 * 2) != hipSuccess) { err = 1; return nullptr; }
    bufs.push_back(p);
    if (spe_launch_wfrag_pack(w, ld, N, p, s) != 0) err = 1;
    return p;
  }
  ~Frags() {
    if (bufs.empty()) return;
    (void)hipStreamSynchronize(s);
    for (void* p : bufs) (void)hipFree(p);
  }
};
}  // namespace

int spe_debug_wfrag_pack(void* stream, const void* w, int ld, int N, void* dst) {
  const int rc = spe_launch_wfrag_pack(w, ld, N, dst, (hipStream_t)stream);
  return rc != 0 ? spe_fail(SPE_E_ARG, "wfrag_pack: bad argument") : 0;
}

int spe_debug_decsa(void* stream, void* tgt, int ldt, int B, int Q, const void* wqk, int ldqk, const float* bqk,
                    const void* wv, int ldv, const float* bv, const void* qpos, const void* wo, int ldo,
                    const float* bo, const float* g, const float* b, float scale) {
  Frags f((hipStream_t)stream);
  DecSaArgs a{};
  a.tgt = tgt; a.ldt = ldt; a.B = B; a.Q = Q;
  a.wqk = f.get(wqk, ldqk, 512); a.bqk = bqk; a.wv = f.get(wv, ldv, 256); a.bv = bv; a.qpos = qpos;
  a.wo = f.get(wo, ldo, 256); a.bo = bo; a.g = g; a.b = b; a.scale = scale;
  if (f.err) return spe_fail(SPE_E_ARG, "decsa: weight packing failed");
  const int rc = spe_launch_decsa(a, (hipStream_t)stream);
  return rc != 0 ? spe_fail(SPE_E_LAUNCH, "decsa launch rejected its arguments") : 0;
}

int spe_debug_decproj(void* stream, void* tgt, int ldt, const void* x, int ldx, int B, int Q, const void* wo, int ldo,
                      const float* bo, const float* g, const float* b) {
  Frags f((hipStream_t)stream);
  DecProjArgs a{};
  a.tgt = tgt; a.ldt = ldt; a.x = x; a.ldx = ldx; a.B = B; a.Q = Q; a.wo = f.get(wo, ldo, 256); a.bo = bo;
  a.g = g; a.b = b;
  if (f.err) return spe_fail(SPE_E_ARG, "decproj: weight packing failed");
  const int rc = spe_launch_decproj(a, (hipStream_t)stream);
  return rc != 0 ? spe_fail(SPE_E_LAUNCH, "decproj launch rejected its arguments") : 0;
}

int spe_debug_decxproj(void* stream, void* tgt, int ldt, float* partial_scratch, int splits, int T, int B, int Q,
                       const void* wv, int ldwv, const float* bv, const void* wo, int ldo, const float* bo,
                       const float* g, const float* b) {
  if (!partial_scratch || T < 1 || B < 0 || Q < 1) return spe_fail(SPE_E_ARG, "bad argument");
  Frags f((hipStream_t)stream);
  DecProjArgs a{};
  a.tgt = tgt; a.ldt = ldt; a.B = B; a.Q = Q; a.wo = f.get(wo, ldo, 256); a.bo = bo; a.g = g; a.b = b;
  const int req = splits > 0 ? splits : spe_xattn_splits(B, Q, T);
  const size_t rows = (size_t)req * B * 8 * Q;  // spe_debug_xattn's scratch layout
  a.pm = partial_scratch; a.pl = partial_scratch + rows; a.pu = partial_scratch + 2 * rows;
  a.splits = spe_xattn_launch_splits(T, req);
  a.wv = f.get(wv, ldwv, 256); a.bv = bv;
  if (f.err) return spe_fail(SPE_E_ARG, "decxproj: weight packing failed");
  const int rc = spe_launch_decproj(a, (hipStream_t)stream);
  return rc != 0 ? spe_fail(SPE_E_LAUNCH, "decxproj launch rejected its arguments") : 0;
}

int spe_debug_decffn(void* stream, const void* x, int ldx, int M, int F, const void* w1, int ld1, const float* b1,
                     const void* w2, int ld2, const float* b2, const float* gamma, const float* beta, void* y, int ldy,
                     float* partial) {
  if (!x || !w1 || !w2 || !y || !partial || M < 0 || F < 256 || F % 256) return spe_fail(SPE_E_ARG, "bad argument");
  Frags f((hipStream_t)stream);
  DecFfnArgs a{};
  a.x = x; a.ldx = ldx; a.M = M; a.F = F; a.b1 = b1; a.partial = partial;
  a.w1 = f.get(w1, ld1, F);
  if (ld2 == 0) {
    a.w2 = w2;
  } else {                                      // W2 packed per 256-wide hidden chunk
    void* p = nullptr;
    if (hipMalloc(&p, (size_t)256 * F * 2) != hipSuccess) return spe_fail(SPE_E_ARG, "decffn: scratch");
    f.bufs.push_back(p);
    for (int c0 = 0; c0 < F; c0 += 256)
      if (spe_launch_wfrag_pack((const char*)w2 + (size_t)c0 * 2, ld2, 256, (char*)p + (size_t)c0 * 256 * 2,
                                (hipStream_t)stream))
        f.err = 1;
    a.w2 = p;
  }
  if (f.err) return spe_fail(SPE_E_ARG, "decffn: weight packing failed");
  FfnArgs r{};
  r.x = x; r.ldx = ldx; r.y = y; r.ldy = ldy; r.M = M; r.D = 256; r.F = F;
  r.b2 = b2; r.gamma = gamma; r.beta = beta; r.splits = F / 256; r.partial = partial;
  int rc = spe_launch_decffn(a, (hipStream_t)stream);
  if (!rc) rc = spe_launch_ffn_reduce_ln(r, (hipStream_t)stream);
  return rc != 0 ? spe_fail(SPE_E_LAUNCH, "decffn launch rejected its arguments") : 0;
}

int spe_debug_decq(void* stream, const void* x, int ldx, int M, int N, const void* w, int ldw, const float* bias,
                   const void* r, int ldr, int period, void* y, int ldy) {
  if (!x || !w || !y || M < 0 || N < 256 || N % 256) return spe_fail(SPE_E_ARG, "bad argument");
  Frags f((hipStream_t)stream);
  DecQArgs a{};
  a.x = x; a.ldx = ldx; a.M = M; a.N = N; a.w = f.get(w, ldw, N); a.bias = bias;
  a.R = r; a.ldr = ldr; a.period = period; a.y = y; a.ldy = ldy;
  if (f.err) return spe_fail(SPE_E_ARG, "decq: weight packing failed");
  const int rc = spe_launch_decq(a, (hipStream_t)stream);
  return rc != 0 ? spe_fail(SPE_E_LAUNCH, "decq launch rejected its arguments") : 0;
}

int spe_debug_btail_perm(int k) { return spe_btail_perm(k); }
int spe_debug_btail_row_perm(int p) { return p >= 0 ? spe_btail_row_perm(p) : -1; }
int spe_debug_btail_wide_perm(int n1, int k) { return spe_btail_wide_perm(n1, k); }

int spe_debug_stempool(void* stream, const void* x, const void* w, int ldw, const float* bias, void* out, int ldo,
                       int B, int S) {
  if (!x || !w || !bias || !out || B < 0) return spe_fail(SPE_E_ARG, "bad argument");
  const int rc = spe_launch_stempool(x, w, ldw, bias, out, ldo, B, S, (hipStream_t)stream);
  return rc != 0 ? spe_fail(SPE_E_LAUNCH, "stempool launch rejected its arguments") : 0;
}

// ---- MobileNetV3 backbone kernels (mbv3.hip)
int spe_debug_dwconv_tiles(int Ho, int Wo) { return Ho > 0 && Wo > 0 ? spe_mb_dwconv_tiles(Ho, Wo) : 0; }

int spe_debug_dwconv(void* stream, int dtype, const void* x, const float* w, const float* bias, void* y,
                     float* pool_partials, int B, int H, int W, int C, int k, int stride, int act) {
  if (!x || !w || !bias || !y) return spe_fail(SPE_E_ARG, "null argument");
  if (dtype != SPE_DTYPE_BF16 && dtype != SPE_DTYPE_F32) return spe_fail(SPE_E_ARG, "bad dtype");
  if (!spe_mb_dwconv_fits(B, H, W, C, k, stride) || (act != MB_ACT_NONE && act != MB_ACT_RELU && act != MB_ACT_HSWISH))
    return spe_fail(SPE_E_ARG, "dwconv: k must be 3 or 5, stride 1 or 2 (even H and W), C a multiple of 8, act 0 / 1 / 4");
  MbDwArgs a{};
  a.in = x; a.out = y; a.w = w; a.bias = bias; a.pool = pool_partials;
  a.B = B; a.H = H; a.W = W; a.C = C; a.k = k; a.stride = stride; a.act = act;
  const int rc = spe_launch_mb_dwconv(a, dtype, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_LAUNCH, "dwconv launch rejected its arguments") : rc;
}

int spe_debug_se_gate(void* stream, const float* pool_partials, int tiles, float inv_hw, const float* w1, const float* b1,
                      const float* w2t, float* scale, int B, int C, int hidden) {
  MbSeArgs a{};
  a.pool = pool_partials; a.tiles = tiles; a.inv_hw = inv_hw;
  a.w1 = w1; a.b1 = b1; a.w2t = w2t; a.scale = scale;
  a.B = B; a.C = C; a.hidden = hidden;
  const int rc = spe_launch_mb_se_gate(a, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_ARG, "se_gate: null argument, C > 1024 or hidden > 256") : rc;
}

int spe_debug_pwconv(void* stream, int dtype, const void* a, int lda, const void* w, int ldw, const float* bias,
                     const float* scale, int rows_per_image, const void* r, int ldr, void* c, int ldc, int M, int N,
                     int K, int act) {
  if (!a || !w || !c) return spe_fail(SPE_E_ARG, "null argument");
  if (dtype != SPE_DTYPE_BF16 && dtype != SPE_DTYPE_F32) return spe_fail(SPE_E_ARG, "bad dtype");
  const int hw = scale ? rows_per_image : M;
  if (M <= 0 || hw <= 0 || M % hw) return spe_fail(SPE_E_ARG, "pwconv: M must be a multiple of rows_per_image");
  MbGemmArgs g{};
  g.A = a; g.lda = lda; g.Bw = w; g.ldb = ldw; g.bias = bias; g.scale = scale;
  g.R = r; g.ldr = ldr; g.C = c; g.ldc = ldc;
  g.M = M; g.N = N; g.K = K;
  g.H = 1; g.W = hw; g.Cin = K; g.KH = 1; g.KW = 1; g.stride = 1; g.pad = 0; g.Ho = 1; g.Wo = hw;
  g.act = act;
  if (!spe_mb_gemm_fits(g)) return spe_fail(SPE_E_ARG, "pwconv: N, K and the row strides must be multiples of 8, act 0 / 1 / 4");
  const int rc = spe_launch_mb_gemm(g, dtype, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_LAUNCH, "pwconv launch rejected its arguments") : rc;
}

int spe_debug_rtdetr_backbone(spe_model* m, void* stream, const float* images, int batch, void* workspace,
                              int64_t workspace_bytes, float* f0, float* f1, float* f2) {
  if (!f0 || !f1 || !f2) return spe_fail(SPE_E_ARG, "null argument");
  const void* f[3];
  int ch[3], hw[3];
  const int rc = spe_rtdetr_backbone(m, (hipStream_t)stream, images, batch, workspace, workspace_bytes, f, ch, hw);
  if (rc) return rc;
  float* out[3] = {f0, f1, f2};
  for (int l = 0; l < 3; ++l) {
    const int e = spe_launch_mb_to_nchw(f[l], out[l], batch, hw[l] * hw[l], ch[l], m->cfg.dtype, (hipStream_t)stream);
    if (e) return spe_fail(e < 0 ? SPE_E_LAUNCH : e, "backbone output conversion failed");
  }
  return 0;
}

int spe_debug_mb_stem(void* stream, int dtype, const float* images, const void* crops, int channels, const float* w,
                      const float* bias, void* y, int B, int S) {
  if ((!images && !crops) || !w || !bias || !y) return spe_fail(SPE_E_ARG, "null argument");
  if (dtype != SPE_DTYPE_BF16 && dtype != SPE_DTYPE_F32) return spe_fail(SPE_E_ARG, "bad dtype");
  const ImageSrc src{crops ? nullptr : images, (const uint8_t*)crops, crops ? channels : 0};
  const int rc = spe_launch_mb_stem(src, w, bias, y, B, S, dtype, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_ARG, "mb_stem: S even (crops: S % 32 == 0, 4-byte aligned, channels 1 / 3)") : rc;
}

// ---- MobileNetV3_Small entry (mbv3s.hip)
int spe_debug_mbs_entry_tiles(int S) { return spe_mbs_entry_fits(1, S) ? spe_mbs_entry_tiles(S) : 0; }

int spe_debug_mbs_entry(void* stream, int dtype, const float* images, const void* crops, int channels,
                        const float* weights, void* pooled, void* skip, void* t2, float* pool_partials, int B, int S) {
  if ((!images && !crops) || !weights || !pooled || !skip || !t2) return spe_fail(SPE_E_ARG, "null argument");
  if (dtype != SPE_DTYPE_BF16 && dtype != SPE_DTYPE_F32) return spe_fail(SPE_E_ARG, "bad dtype");
  if (!spe_mbs_entry_fits(B, S) || (crops && channels != 1 && channels != 3))
    return spe_fail(SPE_E_ARG, "mbs_entry: S a multiple of 16 in [32, 4096], B <= 65535, crops of 1 or 3 channels");
  MbsEntryArgs a{};
  a.src = ImageSrc{crops ? nullptr : images, (const uint8_t*)crops, crops ? channels : 0};
  a.w = weights; a.pooled = pooled; a.skip = skip; a.t2 = t2; a.pool = pool_partials;
  a.B = B; a.S = S;
  const int rc = spe_launch_mbs_entry(a, dtype, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_LAUNCH, "mbs_entry launch rejected its arguments") : rc;
}

// ---- GhostNetV2 backbone kernels (ghostv2.hip)
int spe_debug_ghost_cheap(void* stream, int dtype, const void* x1, int ldx, int xoff, const float* w, const float* bias,
                          void* y, const void* gate, const void* resid, float* pool_partials, int B, int H, int W,
                          int half, int act, int post) {
  if (!x1 || !w || !bias || !y) return spe_fail(SPE_E_ARG, "null argument");
  if (dtype != SPE_DTYPE_BF16 && dtype != SPE_DTYPE_F32) return spe_fail(SPE_E_ARG, "bad dtype");
  GhCheapArgs a{};
  a.x1 = x1; a.ldx = ldx; a.xoff = xoff; a.w = w; a.bias = bias; a.out = y; a.gate = gate; a.resid = resid;
  a.pool = pool_partials;
  a.B = B; a.H = H; a.W = W; a.half = half; a.act = act; a.post = post;
  if (!spe_gh_cheap_fits(a))
    return spe_fail(SPE_E_ARG, "ghost_cheap: half, ldx, xoff must be multiples of 8 (ldx >= xoff + half), act 0 / 1, post 0 / "
                               "1 / 2, even H and W under the gate");
  if ((post == GH_POST_GATE && !gate) || (post == GH_POST_RESIDUAL && !resid))
    return spe_fail(SPE_E_ARG, "ghost_cheap: post 1 needs gate, post 2 needs resid");
  const int rc = spe_launch_gh_cheap(a, dtype, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_LAUNCH, "ghost_cheap launch rejected its arguments") : rc;
}

int spe_debug_dfc_gate(void* stream, int dtype, const void* x, const float* w1, const float* b1, const float* w2,
                       const float* b2, void* gate, int B, int H, int W, int C) {
  if (!x || !w1 || !b1 || !w2 || !b2 || !gate) return spe_fail(SPE_E_ARG, "null argument");
  if (dtype != SPE_DTYPE_BF16 && dtype != SPE_DTYPE_F32) return spe_fail(SPE_E_ARG, "bad dtype");
  if (!spe_gh_dfc_fits(B, H, W, C)) return spe_fail(SPE_E_ARG, "dfc_gate: H, W <= 32, C a multiple of 8");
  GhDfcArgs a{};
  a.x = x; a.gate = gate; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
  a.B = B; a.H = H; a.W = W; a.C = C;
  const int rc = spe_launch_gh_dfc(a, dtype, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_LAUNCH, "dfc_gate launch rejected its arguments") : rc;
}

int spe_debug_se_gate_bias(void* stream, const float* pool_partials, int tiles, float inv_hw, const float* w1,
                           const float* b1, const float* w2t, const float* b2, float* scale, int B, int C, int hidden) {
  if (!b2) return spe_fail(SPE_E_ARG, "null argument");
  MbSeArgs a{};
  a.pool = pool_partials; a.tiles = tiles; a.inv_hw = inv_hw;
  a.w1 = w1; a.b1 = b1; a.w2t = w2t; a.b2 = b2; a.scale = scale;
  a.B = B; a.C = C; a.hidden = hidden;
  const int rc = spe_launch_mb_se_gate(a, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_ARG, "se_gate_bias: null argument, C > 1024 or hidden > 256") : rc;
}

int spe_debug_pool2(void* stream, int dtype, const void* x, void* y, int B, int H, int W, int C) {
  if (!x || !y) return spe_fail(SPE_E_ARG, "null argument");
  if (dtype != SPE_DTYPE_BF16 && dtype != SPE_DTYPE_F32) return spe_fail(SPE_E_ARG, "bad dtype");
  if (!spe_gh_pool2_fits(B, H, W, C)) return spe_fail(SPE_E_ARG, "pool2: H and W must be even, C a multiple of 8");
  const int rc = spe_launch_gh_pool2(x, y, B, H, W, C, dtype, (hipStream_t)stream);
  return rc < 0 ? spe_fail(SPE_E_LAUNCH, "pool2 launch rejected its arguments") : rc;
}

// ---- RT-DETR kernels (rtdetr.hip).  The hooks fill the argument structs and return the launcher's own code
// (0, a hipError_t, or -5 for arguments outside the kernel's contract, refused before any launch).
int spe_debug_rt_resample2x(void* stream, int dtype, const void* in, int ldi, void* out, int ldo, int B, int H, int W,
                            int C, int mode) {
  return spe_launch_resample2x(in, ldi, out, ldo, B, H, W, C, mode, dtype, (hipStream_t)stream);
}

int spe_debug_rt_query_select(void* stream, int dtype, const float* logits, int C, const void* memory, int ldm,
                              const float* anchors, int B, int Q, int D, int levels, const int* lvl_start, int* topk,
                              void* target, int ldt, float* sel_logits, float* sel_anchors) {
  RtSelectArgs a{};
  a.logits = logits; a.C = C; a.memory = memory; a.ldm = ldm; a.anchors = anchors;
  a.B = B; a.Q = Q; a.D = D; a.levels = levels;
  for (int l = 0; l < 5 && l <= levels; ++l) a.lvl_start[l] = lvl_start[l];   // (levels > 4 is refused below)
  a.topk = topk; a.target = target; a.ldt = ldt; a.sel_logits = sel_logits; a.sel_anchors = sel_anchors;
  return spe_launch_query_select(a, dtype, (hipStream_t)stream);
}

int spe_debug_rt_qpos_hidden(void* stream, int dtype, const float* ref, const float* w0, const float* b0, void* out,
                             int rows, int H) {
  return spe_launch_qpos_hidden(ref, w0, b0, out, rows, H, dtype, (hipStream_t)stream);
}

int spe_debug_rt_head_finish(void* stream, int dtype, int rows, int Q, int C, const float* hs, const float* cls_w,
                             const float* cls_b, const void* h2, int ld_h2, const float* box_w2, const float* box_b2,
                             const float* sig_w2, const float* sig_b2, const float* pt_add, int pt_add_invsig,
                             float* logits, float* probs, float* points, const float* clip_bbox, float* points_px,
                             float* log_sigmas, float* sigmas) {
  RtHeadArgs a{};
  a.rows = rows; a.Q = Q; a.C = C;
  a.hs = hs; a.cls_w = cls_w; a.cls_b = cls_b;
  a.h2 = h2; a.ld_h2 = ld_h2;
  a.box_w2 = box_w2; a.box_b2 = box_b2; a.sig_w2 = sig_w2; a.sig_b2 = sig_b2;
  a.pt_add = pt_add; a.pt_add_invsig = pt_add_invsig;
  a.logits = logits; a.probs = probs; a.points = points;
  a.clip_bbox = clip_bbox; a.points_px = points_px;
  a.log_sigmas = log_sigmas; a.sigmas = sigmas;
  return spe_launch_head_finish(a, dtype, (hipStream_t)stream);
}

int spe_debug_rt_msdeform(void* stream, int dtype, const void* value, int ldv, const float* so_aw, int ld_so,
                          const float* ref, void* out, int ldo, int rows, int Q, int heads, int levels, int points,
                          const int* lvl_h, const int* lvl_w, const int* lvl_rows0) {
  RtDeformArgs a{};
  a.value = value; a.ldv = ldv; a.so_aw = so_aw; a.ld_so = ld_so; a.ref = ref; a.out = out; a.ldo = ldo;
  a.rows = rows; a.Q = Q; a.heads = heads; a.levels = levels; a.points = points;
  for (int l = 0; l < 4 && l < levels; ++l) {                                   // (levels > 4 is refused below)
    a.lvl_h[l] = lvl_h[l]; a.lvl_w[l] = lvl_w[l]; a.lvl_rows0[l] = lvl_rows0[l];
  }
  return spe_launch_msdeform(a, dtype, (hipStream_t)stream);
}

int spe_debug_rt_deform_map(void* stream, const float* so_aw, int ld_so, const float* ref, int rows, int Q, int heads,
                            int levels, int points, const int* lvl_h, const int* lvl_w, float* map, float* loc,
                            float* weights) {
  RtDeformMapArgs a{};
  a.so_aw = so_aw; a.ld_so = ld_so; a.ref = ref; a.map = map; a.loc = loc; a.weights = weights;
  a.rows = rows; a.Q = Q; a.heads = heads; a.levels = levels; a.points = points;
  for (int l = 0; l < 4 && l < levels; ++l) {                                   // (levels > 4 is refused below)
    a.lvl_h[l] = lvl_h[l]; a.lvl_w[l] = lvl_w[l];
    a.lvl_start[l + 1] = a.lvl_start[l] + lvl_h[l] * lvl_w[l];
  }
  return spe_launch_deform_map(a, (hipStream_t)stream);
}

// ---- DETR stem, neck and head helpers (elementwise.hip, heads.hip).  Like the rt hooks: the launcher's own code
// (0, a hipError_t, -5 / -6 for arguments outside the kernel's contract, refused before any launch).
int spe_debug_pack_input(void* stream, int dtype, const float* images_f32, const void* crops_u8, int channels, void* out,
                         int B, int S, int cpad, float* amax) {
  if (!out || B < 0 || S < 1) return spe_fail(SPE_E_ARG, "bad argument");
  if (dtype != SPE_DTYPE_BF16 && dtype != SPE_DTYPE_F32) return spe_fail(SPE_E_ARG, "bad dtype");
  const ImageSrc src{images_f32, (const uint8_t*)crops_u8, channels};
  return spe_launch_pack_input(src, out, B, S, dtype, (hipStream_t)stream, amax, cpad);
}

int spe_debug_pack_input_pad4(void* stream, const float* images_f32, const void* crops_u8, int channels, void* out, int B,
                              int S) {
  if (!out || B < 0 || S < 1) return spe_fail(SPE_E_ARG, "bad argument");
  const ImageSrc src{images_f32, (const uint8_t*)crops_u8, channels};
  return spe_launch_pack_input_pad4(src, out, B, S, (hipStream_t)stream);
}

int spe_debug_maxpool3s2(void* stream, int dtype, const void* in, void* out, int B, int H, int W, int C, int ldo) {
  if (!in || !out || B < 0 || H < 1 || W < 1 || C < 1) return spe_fail(SPE_E_ARG, "bad argument");
  if (dtype != SPE_DTYPE_BF16 && dtype != SPE_DTYPE_F32) return spe_fail(SPE_E_ARG, "bad dtype");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;     // (forward.cpp's)
  return spe_launch_maxpool3s2(in, out, B, H, W, C, Ho, Wo, dtype, (hipStream_t)stream, ldo);
}

int spe_debug_upsample2x(void* stream, int dtype, const void* in, void* out, int B, int H, int W, int C) {
  if (!in || !out || B < 0 || H < 1 || W < 1 || C < 1) return spe_fail(SPE_E_ARG, "bad argument");
  if (dtype != SPE_DTYPE_BF16 && dtype != SPE_DTYPE_F32) return spe_fail(SPE_E_ARG, "bad dtype");
  return spe_launch_upsample2x(in, out, B, H, W, C, dtype, (hipStream_t)stream);
}

int spe_debug_heads(void* stream, const float* hs, int B, int Q, int D, const float* cls_wt, const float* cls_b,
                    const float* pt_w0t, const float* pt_b0, const float* pt_w1t, const float* pt_b1, const float* pt_w2t,
                    const float* pt_b2, const float* sg_w0t, const float* sg_b0, const float* sg_w1t, const float* sg_b1,
                    const float* sg_w2t, const float* sg_b2, const float* clip_bbox, float* logits, float* points,
                    float* probs, float* points_px, float* log_sigmas, float* sigmas) {
  if (!hs || !cls_wt || !cls_b || !pt_w0t || !pt_b0 || !pt_w1t || !pt_b1 || !pt_w2t || !pt_b2 || !logits || !points ||
      B < 0 || Q < 1)
    return spe_fail(SPE_E_ARG, "bad argument");
  if (sg_w0t && (!sg_b0 || !sg_w1t || !sg_b1 || !sg_w2t || !sg_b2))
    return spe_fail(SPE_E_ARG, "heads: a sigma head needs its three weight / bias pairs");
  HeadArgs a{};
  a.hs = hs; a.B = B; a.Q = Q; a.D = D;
  a.cls_wt = cls_wt; a.cls_b = cls_b;
  a.pt_w0t = pt_w0t; a.pt_b0 = pt_b0; a.pt_w1t = pt_w1t; a.pt_b1 = pt_b1; a.pt_w2t = pt_w2t; a.pt_b2 = pt_b2;
  a.sg_w0t = sg_w0t; a.sg_b0 = sg_b0; a.sg_w1t = sg_w1t; a.sg_b1 = sg_b1; a.sg_w2t = sg_w2t; a.sg_b2 = sg_b2;
  a.clip_bbox = clip_bbox;
  a.logits = logits; a.points = points; a.probs = probs; a.points_px = points_px;
  a.log_sigmas = log_sigmas; a.sigmas = sigmas;
  return spe_launch_heads(a, (hipStream_t)stream);
}

}  // extern "C"
