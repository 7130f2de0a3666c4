// Native runtime of the keypoint-set predictor, part 2: the launch sequence of one forward
// pass (REV/models/detr_speed.py:59-92 -> backbone.py:133-149 -> transformer.py:51-63 ->
// heads + PostProcess) on one HIP stream (the solver / score entry points are in ops_capi.cpp).  No
// allocation or synchronisation happens inside spe_forward / spe_pnp_batch / spe_speed_score, so a caller
// may capture them into a hipGraph.  Every launch goes through run_gemm / run_attn / run_other (launch.cpp),
// which bracket it with HIP events when the per-launch profiler is on (bench roofline).
#include <hip/hip_runtime.h>

#include <cmath>

#include "launch.h"
#include "model_state.h"
#include "spe_common.h"

#define fail spe_fail
// a function of this file that failed has recorded the launch that did (CK): pass its code up unchanged
#define TRY(x)                         \
  do {                                 \
    if (const int _r = (x)) return _r; \
  } while (0)

namespace {

// spe_forward_attention's taps (attn_map.hip): the head-averaged attention probabilities of encoder layer
// enc_layer's self-attention into enc_map [B][T][T] and of decoder layer dec_layer's cross-attention into
// dec_map [B][Q][T]; a null map skips its tap.  Layer indices are resolved (>= 0) by the entry point.
struct AttnTap {
  int enc_layer, dec_layer;
  float *enc_map, *dec_map;
};

// One forward call: the model, the workspace plan and the call's sizes.  What flows between stages flows
// through the workspace (src, srcpos, ck / cvt, the activation-scale slots), never through this struct.
struct Fwd {
  spe_model* m;
  Ws w;
  char* ws;
  hipStream_t s;
  int B, S, F, T, d, ff, Q, L, Mt, Mq, dt;
  float scale;
  // fp32h3: each tensor a GEMM reads carries a device max |x| (the producer's published maximum,
  // or a bound), the scale input of the scaled fp16 split (gemm.hip gemm_h3d).  Slots: backbone
  // [0, SPE_AMAX_BB), the neck output (the encoder's first input) at SPE_AMAX_BB - 1, transformer
  // [SPE_AMAX_BB, SPE_AMAX_SLOTS); each stage zeroes its own range first.
  float* amx;
  LedgerScope& ledger;
  const AttnTap* tap;        // spe_forward_attention only, else null
  void* P(size_t off) const { return ws + off; }
  float* slot(int i) const { return amx ? amx + i : nullptr; }
};

// a stage zeroes its slot range before its first launch
int zero_slots(Fwd& f, int first, int n) {
  if (!f.amx) return 0;
  CK((int)hipMemsetAsync(f.amx + first, 0, n * 4, f.s));
  f.ledger.zeroed(first, n);
  return 0;
}

bool use_fused_ffn(const spe_model* m) {
  return m->cfg.dtype == SPE_DTYPE_BF16 && m->cfg.hidden_dim == 256 && m->cfg.dim_feedforward % 32 == 0;
}

// x = LayerNorm(x + a . W^T + b): the GEMM with the residual x into tmp, the LayerNorm back into x
int linear_residual_ln(Fwd& f, const char* gemm_kind, const char* ln_kind, const Conv& c, const void* a, int lda,
                       const float* a_amax, int M, void* x, void* tmp, const float* lg, const float* lb) {
  GemmArgs g = linear_args(c, a, lda, M, tmp, f.d);
  g.R = x; g.ldr = f.d;
  g.amax_a = a_amax;
  CK(run_gemm(f.m, gemm_kind, g, GEMM_LINEAR, f.s));
  CK(run_layernorm(f.m, ln_kind, tmp, lg, lb, x, nullptr, M, f.d, f.dt, f.s));
  return 0;
}

// linear1 + ReLU publishing max |hidden| into `h_amax`, linear2 + residual reading it, the LayerNorm
int unfused_ffn(Fwd& f, const char* kind1, const char* kind2, const char* ln_kind, const Conv& l1, const Conv& l2,
                void* x, const float* x_amax, int M, void* hidden, float* h_amax, void* tmp, const float* lg,
                const float* lb) {
  GemmArgs g = linear_args(l1, x, f.d, M, hidden, f.ff);
  g.act = ACT_RELU;
  g.amax_a = x_amax; g.amax_c = h_amax;
  CK(run_gemm(f.m, kind1, g, GEMM_LINEAR, f.s));
  return linear_residual_ln(f, kind2, ln_kind, l2, hidden, f.ff, h_amax, M, x, tmp, lg, lb);
}

// ---------------- backbone (REV/models/backbone.py:133-149)

// what one bottleneck block hands to the next
struct BlockIn {
  size_t x;                  // the block's input (w.pool aliases bufA)
  int ld, H;
  const float* amax;
  bool t1_ready;             // this block's conv1 ran in the previous block's tail
  bool src_ready;            // stride-16 model: input_proj ran in the last block's tail (src is written, x is not)
  bool x_compact;            // x holds only the even pixels, [B][H/2][H/2][ld]: all this block's stride-2 downsample reads
};

// a fused bottleneck tail (btail.hip, btail_wide.hip): y = relu(c3 over A (+ R)), then z = the second 1x1 conv c2
// (the next block's permuted conv1, or the permuted input_proj) over y; the caller sets y and what its form adds
BtailArgs btail_args(const Conv& c3, const void* A, int lda, const void* R, const Conv& c2, void* z, int ldz, int M) {
  BtailArgs t{};
  t.A = A; t.lda = lda; t.k1 = c3.K; t.R = R; t.ldr = c3.N;
  t.w3 = c3.w; t.ld3 = c3.Kpad; t.b3 = c3.bias; t.ldy = c3.N; t.n1 = c3.N;
  t.w1 = c2.w; t.ld1 = c2.Kpad; t.b1 = c2.bias; t.z = z; t.ldz = ldz; t.n2 = c2.N;
  t.M = M;
  return t;
}

// conv3 (+ residual R) + relu of a block: with the next block's conv1 as one launch (btail.hip, or
// btail_wide.hip for layers 2 and 3) when the next block carries permuted conv1 weights (registry.cpp c1p) and the shapes are served
// (*tailed), else the GEMM.  c3 over A is either Block::c3 over t2 or Block::c3ds over [t2 | x].
// Ho > 0: the M = B * Ho * Ho rows of `out` have one more reader only, the next block's stride-2 downsample, so
// the tail may store just the even pixels (*compact; btail.hip YC, behind SPE_BTAIL_YCOMPACT).
int conv3_tail_or_gemm(Fwd& f, const Block* nb, const Conv& c3, const void* A, int lda, const float* a_amax,
                       const void* R, void* out, float* out_amax, int M, bool* tailed, int Ho = 0,
                       bool* compact = nullptr) {
  spe_model* m = f.m;
  int rc = 1;
  if (nb) {
    BtailArgs t = btail_args(c3, A, lda, R, nb->c1p, f.P(f.w.t1), nb->c1.N, M);
    t.y = out;
    t.rows = m->btail_rows;
    // (below one 16-row tile per wave of the persistent grid the launch is latency, not store traffic: y stays
    // whole there, and the launch tables of the small golden cases stay as recorded)
    t.ycompact = compact && Ho > 0 && m->btail_ycompact && M >= 16 * 8 * spe_cu_count(); t.H = t.W = Ho;
    const bool yc = c3.N == 256 && spe_btail_ycompact_serves(t);
    const double flops = 2.0 * M * ((double)c3.N * c3.K + (double)nb->c1.N * c3.N);
    const double bytes = ((double)M * (c3.K + c3.N / (yc ? 4.0 : 1.0) + nb->c1.N) + (R ? (double)M * c3.N : 0.0)) * m->esz;
    if (compact) *compact = false;
    if (c3.N == 256) {
      rc = run_other(m, "conv.1x1", flops, bytes, f.s, [&] { return spe_launch_btail(t, f.s); });
      if (compact) *compact = rc == 0 && yc;
    } else if (spe_btail_wide_serves(t) && spe_btail_wide_tiles(t) >= spe_cu_count() / 2) {
      // layers 2 and 3 (btail_wide.hip), every boundary measured faster than its two launches in the
      // profiled B = 64 step (fused vs conv3 + conv1, ms): layer 2 inner 0.122 vs 0.170, layer 2 -> 3
      // 0.162 vs 0.192, layer 3 block 0 -> 1 0.083 vs 0.111, layer 3 inner 0.082 vs 0.094
      // (profiles/btail_wide_ab_ms_per_step.json).  Below half a tile per CU (not measured) the two
      // GEMMs stay: they also split the columns over the chip.
      rc = run_other(m, "conv.1x1", flops, bytes, f.s, [&] { return spe_launch_btail_wide(t, f.s); });
    }
    if (rc != 0 && rc != 1) CK(rc);   // 1 = shapes not served: the GEMM below
  }
  if (rc == 1) {
    GemmArgs g = linear_args(c3, A, lda, M, out, c3.N);
    if (R) { g.R = R; g.ldr = c3.N; }
    g.act = ACT_RELU;
    g.amax_a = a_amax; g.amax_c = out_amax;
    CK(run_gemm(m, "conv.1x1", g, GEMM_LINEAR, f.s));
  }
  *tailed = rc == 0;
  return 0;
}

// The stride-16 model's last bottleneck (bf16): conv3 + identity + relu with input_proj as the tail's second
// product, straight into src; the 1024-channel block output, which nobody else reads, is never stored
// (btail_wide.hip's final form).  Taken under the rule of layers 2 and 3 above: served, and at least half a
// tile per CU; else *done stays false and the caller runs conv3 and input_proj as two GEMMs.
// Behind SPE_BTAIL_PROJ=1 only: measured at B = 64, 448^2 (262 tiles) the fused launch was not faster than the
// two GEMMs (backbone stage 3.605 against 3.600 ms, profiles/backbone_s16_vs_s8.json), so by the rule above
// the two GEMMs are the default.
int final_tail(Fwd& f, const Conv& c3, const void* A, int lda, const void* R, int M, bool* done) {
  spe_model* m = f.m;
  *done = false;
  if (!m->ipp.w || !spe_btail_wide_proj_enabled()) return 0;
  const BtailArgs t = btail_args(c3, A, lda, R, m->ipp, f.P(f.w.src), f.d, M);   // (y stays null: never stored)
  if (t.n2 != f.d || !spe_btail_wide_proj_serves(t) || spe_btail_wide_tiles(t) < spe_cu_count() / 2) return 0;
  const double flops = 2.0 * M * ((double)c3.N * c3.K + (double)t.n2 * c3.N);
  const double bytes = ((double)M * (c3.K + t.n2) + (R ? (double)M * c3.N : 0.0)) * m->esz;
  const int rc = run_other(m, "conv.1x1", flops, bytes, f.s, [&] { return spe_launch_btail_wide_proj(t, false, f.s); });
  if (rc != 0 && rc != 1) CK(rc);
  *done = rc == 0;
  return 0;
}

// what both bottleneck forms derive from block bi and its input: where the output goes, its edge Ho, and a first
// block's downsample conv over the whole input into w.ds (the 1x1 as a linear GEMM, the stride-2 1x1 as a conv)
struct BlockPlan {
  size_t outbuf;
  int Ho, ds_mode;
  const char* ds_kind;
  GemmArgs ds;
};
BlockPlan block_plan(const Fwd& f, size_t bi, const BlockIn& in) {
  const Ws& w = f.w;
  const Block& blk = f.m->blocks[bi];
  // layer1: blocks 0-2, layer2: 3-6 (its output xs8 is kept for the neck; the stride-16 model has none), layer3: 7-12
  const bool keep8 = bi == 6 && f.m->backbone != SPE_BACKBONE_RESNET50_S16;
  BlockPlan p{keep8 ? w.xs8 : (in.x == w.bufA ? w.bufB : w.bufA), (in.H + 2 - 3) / blk.stride + 1, GEMM_LINEAR, "conv.1x1", {}};
  if (blk.has_ds && blk.stride == 1) p.ds = linear_args(blk.ds, f.P(in.x), in.ld, f.B * in.H * in.H, f.P(w.ds), blk.ds.N);
  if (blk.has_ds && blk.stride != 1) {
    p.ds_mode = GEMM_CONV; p.ds_kind = "conv.1x1s2";
    p.ds = conv_args(blk.ds, f.P(in.x), f.B, in.H, in.H, f.P(w.ds), blk.ds.N);
  }
  return p;
}

// bottleneck block bi over `in`, which becomes the block's output; activation-scale slots 2 + 3 bi ...
int bottleneck(Fwd& f, size_t bi, BlockIn& in) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  hipStream_t s = f.s;
  const int B = f.B, H = in.H;
  const Block& blk = m->blocks[bi];
  const BlockPlan bp = block_plan(f, bi, in);
  const size_t outbuf = bp.outbuf; const int Ho = bp.Ho;
  // bf16: layer1 block 0's conv3 + downsample run as one GEMM over [conv2 output | pool output]
  // (Block::c3ds): conv2 writes the left half of that concatenation (w.ds region, row stride c3ds.K),
  // the max-pool wrote the right half (backbone_stage)
  const bool fused = bi == 0 && blk.c3ds.w != nullptr;
  const Block* nb = bi + 1 < m->blocks.size() && m->blocks[bi + 1].c1p.w ? &m->blocks[bi + 1] : nullptr;
  const bool s16bb = m->backbone == SPE_BACKBONE_RESNET50_S16;
  float* const t1_amax = f.slot(2 + 3 * (int)bi);
  float* const t2_amax = f.slot(2 + 3 * (int)bi + 1);
  float* const out_amax = f.slot(2 + 3 * (int)bi + 2);
  if (!in.t1_ready) {  // conv1 1x1 + bn1 + relu
    GemmArgs g = linear_args(blk.c1, f.P(in.x), in.ld, B * H * H, f.P(w.t1), blk.c1.N);
    g.act = ACT_RELU;
    g.amax_a = in.amax; g.amax_c = t1_amax;
    CK(run_gemm(m, "conv.1x1", g, GEMM_LINEAR, s));
  }
  {  // conv2 3x3 (stride on the 3x3, ResNet v1.5) + bn2 + relu
    GemmArgs g = conv_args(blk.c2, f.P(w.t1), B, H, H, fused ? f.P(w.ds) : f.P(w.t2), fused ? in.ld : blk.c2.N);
    g.act = ACT_RELU;
    g.amax_a = t1_amax; g.amax_c = t2_amax;
    CK(run_gemm(m, "conv.3x3", g, GEMM_CONV, s));
  }
  if (fused) {  // relu(W3 t2 + Wds x + b3 + bds) over the concatenation
    TRY(conv3_tail_or_gemm(f, blk.c3ds.N == 256 ? nb : nullptr, blk.c3ds, f.P(w.ds), in.ld, nullptr, nullptr,
                           f.P(outbuf), nullptr, B * Ho * Ho, &in.t1_ready));
  } else {
    size_t res = in.x;
    if (blk.has_ds) {
      if (blk.stride == 2 && in.x_compact) {
        // the previous tail stored exactly the pixels this conv reads, densely: the same conv kernel at stride 1
        // over [B][Ho][Ho] (the same rows in the same K order, so the same bits; the streaming GEMM_LINEAR
        // kernels sum K in another order and were not tried)
        Conv d1 = blk.ds;
        d1.stride = 1;
        GemmArgs g = conv_args(d1, f.P(in.x), B, Ho, Ho, f.P(w.ds), blk.ds.N);
        CK(run_gemm(m, "conv.1x1s2", g, GEMM_CONV, s));
      } else {
        GemmArgs g = bp.ds;
        g.amax_a = in.amax;
        CK(run_gemm(m, bp.ds_kind, g, bp.ds_mode, s));
      }
      res = w.ds;
    }
    // conv3 1x1 + bn3 + residual + relu (+ the next block's conv1, btail.hip; + input_proj after the
    // stride-16 model's last block)
    if (s16bb && bi + 1 == m->blocks.size())
      TRY(final_tail(f, blk.c3, f.P(w.t2), blk.c2.N, f.P(res), B * Ho * Ho, &in.src_ready));
    // The block output has two readers, the next block's conv1 and its residual path.  When that path is a
    // stride-2 downsample (and conv1 runs in the tail) nothing reads the odd pixels: every model (both
    // backbones; only bf16 models have tails) walks its blocks through this function alone, the neck reads
    // block 6's output (xs8, which is why that block is excluded) and the last block's, and the attention
    // taps and the activation-scale slots (fp32h3 only) read no block output.
    const bool ds_only = nb && nb->stride == 2 && nb->has_ds && outbuf != w.xs8;
    in.x_compact = false;
    if (!in.src_ready)
      TRY(conv3_tail_or_gemm(f, nb, blk.c3, f.P(w.t2), blk.c2.N, t2_amax, f.P(res), f.P(outbuf), out_amax, B * Ho * Ho,
                             &in.t1_ready, ds_only ? Ho : 0, &in.x_compact));
    in.amax = out_amax;
  }
  in.ld = blk.c3.N;
  in.H = Ho;
  in.x = outbuf;
  return 0;
}

// ---------------- the GroupNorm backbone (SPE_MODEL_GROUP_NORM; REV/models/backbone.py:168-181, --bn group_bn)
//
// Every body conv runs with an identity epilogue (no bias, no ReLU, no residual) and nn.GroupNorm(32, C) follows it
// as two launches over the conv's output, in place (groupnorm.hip): norm.gn.stats, then norm.gn.apply with the
// block's residual and ReLU.  No fused stem + pool and no fused bottleneck tail is taken: a norm sits inside each.

// x [B*H*H][ld] = relu?(GroupNorm(x; a) (+ res)) over C channels
int group_norm(Fwd& f, void* x, int ld, int H, int C, const GnAffine& a, const void* res, int ldr, bool relu) {
  spe_model* m = f.m;
  GroupNormArgs g{};
  g.x = x; g.ldx = ld; g.res = res; g.ldr = ldr; g.gamma = a.g; g.beta = a.b; g.y = x; g.ldy = ld;
  g.B = f.B; g.H = H; g.W = H; g.C = C; g.relu = relu; g.part = (float*)f.P(f.w.gn);
  const double elems = (double)f.B * H * H * C, part = (double)spe_gn_scratch_bytes(f.B, H, H, C);
  CK(run_other(m, "norm.gn.stats", 0.0, elems * m->esz + part, f.s, [&] { return spe_launch_gn_stats(g, f.dt, f.s); }));
  CK(run_other(m, "norm.gn.apply", 0.0, elems * m->esz * (res ? 3.0 : 2.0) + part, f.s,
               [&] { return spe_launch_gn_apply(g, f.dt, f.s); }));
  return 0;
}

// a conv with nothing behind its accumulator
int bare_gemm(Fwd& f, const char* kind, GemmArgs g, int mode) {
  g.bias = nullptr;
  return run_gemm(f.m, kind, g, mode, f.s);
}

// bottleneck block bi over `in`: conv1 -> GN + ReLU; conv2 -> GN + ReLU; conv3 -> GN (+ the identity, or the GN'd
// downsample branch) + ReLU (torchvision Bottleneck.forward with norm_layer = MyGroupNorm)
int bottleneck_gn(Fwd& f, size_t bi, BlockIn& in) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  const int B = f.B, H = in.H;
  const Block& blk = m->blocks[bi];
  const BlockPlan bp = block_plan(f, bi, in);
  const size_t outbuf = bp.outbuf; const int Ho = bp.Ho;
  CK(bare_gemm(f, "conv.1x1", linear_args(blk.c1, f.P(in.x), in.ld, B * H * H, f.P(w.t1), blk.c1.N), GEMM_LINEAR));
  TRY(group_norm(f, f.P(w.t1), blk.c1.N, H, blk.c1.N, blk.n1, nullptr, 0, true));
  CK(bare_gemm(f, "conv.3x3", conv_args(blk.c2, f.P(w.t1), B, H, H, f.P(w.t2), blk.c2.N), GEMM_CONV));
  TRY(group_norm(f, f.P(w.t2), blk.c2.N, Ho, blk.c2.N, blk.n2, nullptr, 0, true));
  size_t res = in.x;
  int ldr = in.ld;
  if (blk.has_ds) {
    CK(bare_gemm(f, bp.ds_kind, bp.ds, bp.ds_mode));
    TRY(group_norm(f, f.P(w.ds), blk.ds.N, Ho, blk.ds.N, blk.nds, nullptr, 0, false));
    res = w.ds;
    ldr = blk.ds.N;
  }
  CK(bare_gemm(f, "conv.1x1", linear_args(blk.c3, f.P(w.t2), blk.c2.N, B * Ho * Ho, f.P(outbuf), blk.c3.N), GEMM_LINEAR));
  TRY(group_norm(f, f.P(outbuf), blk.c3.N, Ho, blk.c3.N, blk.n3, f.P(res), ldr, true));
  in.ld = blk.c3.N;
  in.H = Ho;
  in.x = outbuf;
  return 0;
}

// s8_latern | s16_latern -> concat, output_conv, input_proj -> src [B*T, d] and its scale slot
int neck(Fwd& f, size_t xs16, const float* xs8_amax, const float* xs16_amax) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  hipStream_t s = f.s;
  const int B = f.B, S = f.S, F = f.F, T = f.T, d = f.d, dt = f.dt;
  const int slot0 = 2 + 3 * (int)m->blocks.size();
  float* const cat_amax = f.slot(slot0);
  float* const src_amax = f.slot(SPE_AMAX_BB - 1);
  {  // s8_latern 1x1 512->256 into channels [0,256) of the concat buffer
    GemmArgs g = linear_args(m->s8, f.P(w.xs8), 512, B * T, f.P(w.cat), 512);
    g.bias = nullptr;
    g.amax_a = xs8_amax; g.amax_c = cat_amax;
    CK(run_gemm(m, "conv.neck", g, GEMM_LINEAR, s));
  }
  if (spe_use_upconv(m)) {
    // s16_latern(up16sto8s(xs16)) at the low resolution: Z = xs16 . [W_t]^T for the 9 taps
    // (w.up holds Z [B*(S/16)^2][9*256]), then the bilinear combine into channels [256,512)
    const int h = S / 16, nz = m->s16taps.N;
    GemmArgs g = linear_args(m->s16taps, f.P(xs16), 1024, B * h * h, f.P(w.up), nz);
    // the combine sums nine bilinear interpolations of Z (each a convex combination): its output
    // is bounded by 9 max |Z|, published into the concat's slot
    g.amax_a = xs16_amax; g.amax_c = cat_amax; g.amax_c_mul = 9.f;
    CK(run_gemm(m, "conv.neck", g, GEMM_LINEAR, s));
    const double by = ((double)B * h * h * nz + (double)B * 4 * h * h * 256) * m->esz;
    CK(run_other(m, "eltwise.upconv", 0.0, by, s, [&] {
      return spe_launch_upconv_combine(f.P(w.up), (char*)f.P(w.cat) + 256 * m->esz, 512, B, h, h, 256, dt, s);
    }));
  } else {
    CK(run_other(m, "eltwise.upsample", 0.0, (double)B * 1024 * 5 * (S / 16) * (S / 16) * m->esz, s,
                 [&] { return spe_launch_upsample2x(f.P(xs16), f.P(w.up), B, S / 16, S / 16, 1024, dt, s); }));
    // s16_latern 3x3 1024->256 into channels [256,512)
    GemmArgs g = conv_args(m->s16, f.P(w.up), B, F, F, (char*)f.P(w.cat) + 256 * m->esz, 512);
    g.bias = nullptr;
    g.amax_a = xs16_amax; g.amax_c = cat_amax;          // (bilinear upsampling keeps max |x|)
    CK(run_gemm(m, "conv.neck", g, GEMM_CONV, s));
  }
  if (spe_use_neckfold(m)) {  // input_proj . output_conv as one 3x3 conv 512->256 -> src [B*T, 256]
    GemmArgs g = conv_args(m->neckip, f.P(w.cat), B, F, F, f.P(w.src), d);
    g.amax_a = cat_amax; g.amax_c = src_amax;
    CK(run_gemm(m, "conv.neck", g, GEMM_CONV, s));
  } else {
    float* const neck_amax = f.slot(slot0 + 1);
    {  // output_conv 3x3 512->512 + bias
      GemmArgs g = conv_args(m->outc, f.P(w.cat), B, F, F, f.P(w.neck), 512);
      g.amax_a = cat_amax; g.amax_c = neck_amax;
      CK(run_gemm(m, "conv.neck", g, GEMM_CONV, s));
    }
    {  // input_proj 1x1 512->256 + bias -> src [B*T, 256] (token order h*W+w)
      GemmArgs g = linear_args(m->inproj, f.P(w.neck), 512, B * T, f.P(w.src), d);
      g.amax_a = neck_amax; g.amax_c = src_amax;
      CK(run_gemm(m, "gemm.input_proj", g, GEMM_LINEAR, s));
    }
  }
  return 0;
}

int backbone_stage(Fwd& f, const ImageSrc& images) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  hipStream_t s = f.s;
  const int B = f.B, S = f.S, dt = f.dt;
  TRY(zero_slots(f, 0, SPE_AMAX_BB));
  const bool pairs = m->esz == 2 && m->stem.Cin == 4;  // bf16: pair-packed stem (registry.cpp)
  float* const x0_amax = f.slot(0);
  if (pairs)
    CK(run_other(m, "eltwise.pack", 0.0, (double)B * S * S * 12 + (double)B * (S + 6) * (S + 6) * 8, s,
                 [&] { return spe_launch_pack_input_pad4(images, f.P(w.x0), B, S, s); }));
  else
    CK(run_other(m, "eltwise.pack", 0.0, (double)B * S * S * (12 + m->stem.Cin * m->esz), s,
                 [&] { return spe_launch_pack_input(images, f.P(w.x0), B, S, dt, s, x0_amax, m->stem.Cin); }));
  CK(ledger_use(nullptr, x0_amax, "eltwise.pack"));
  const int H = S / 2;
  float* const stem_amax = f.slot(1);
  const int Hp = (H + 2 - 3) / 2 + 1;
  // bf16: layer1 block 0's conv3 + downsample run as one GEMM over [conv2 output | pool output]
  // (Block::c3ds), so the max-pool writes the right half of that concatenation (w.ds region,
  // row stride c3ds.K) and conv2 the left half
  const Block& b0 = m->blocks[0];
  const bool fuse0 = b0.c3ds.w != nullptr;
  const int uld = fuse0 ? b0.c3ds.K : 64;
  const size_t pool_at = fuse0 ? w.ds + (size_t)b0.c2.N * m->esz : w.pool;
  // the unfused stem: the 7x7/2 conv as a GEMM into w.stem (the pair-packed input carries its border), its max-pool
  const int Sin = pairs ? S + 6 : S;
  auto stem_args = [&] { return conv_args(m->stem, f.P(w.x0), B, Sin, Sin, f.P(w.stem), 64); };
  auto maxpool = [&] {
    return run_other(m, "eltwise.maxpool", 0.0, (double)B * 64 * (H * H + Hp * Hp) * m->esz, s, [&] {
      return spe_launch_maxpool3s2(f.P(w.stem), f.P(pool_at), B, H, H, 64, Hp, Hp, dt, s, uld);
    });
  };
  if (m->group_norm) {
    // GN + ReLU between the two, in place over the stem output
    CK(bare_gemm(f, "conv.stem", stem_args(), GEMM_CONV));
    TRY(group_norm(f, f.P(w.stem), 64, H, 64, m->stem_n, nullptr, 0, true));
    CK(maxpool());
  } else if (pairs && spe_stempool_enabled() && spe_stempool_fits(S)) {
    // stem + bias + ReLU + max-pool in one pass (stempool.hip): the stem output stays in registers
    const double flops = 2.0 * B * H * H * 64 * 7 * 8 * 4;
    const double bytes = (double)B * (S + 6) * (S + 6) * 8 + (double)B * Hp * Hp * 64 * m->esz;
    CK(run_other(m, "conv.stem", flops, bytes, s, [&] {
      return spe_launch_stempool(f.P(w.x0), m->stem.w, m->stem.Kpad, m->stem.bias, f.P(pool_at), uld, B, S, s);
    }));
  } else {
    GemmArgs g = stem_args();
    g.act = ACT_RELU;
    g.amax_a = x0_amax; g.amax_c = stem_amax;
    CK(run_gemm(m, "conv.stem", g, GEMM_CONV, s));
    CK(maxpool());
  }
  BlockIn x{pool_at, uld, Hp, stem_amax, false, false, false};  // (the max-pool's maximum is the stem's)
  const float* xs8_amax = nullptr;
  for (size_t bi = 0; bi < m->blocks.size(); ++bi) {
    TRY(m->group_norm ? bottleneck_gn(f, bi, x) : bottleneck(f, bi, x));
    if (bi == 6) xs8_amax = x.amax;
  }
  if (m->backbone != SPE_BACKBONE_RESNET50_S16)
    return neck(f, x.x, xs8_amax, x.amax);               // x: xs16 [B, S/16, S/16, 1024]
  // the plain ResNet-50 (REV/models/backbone.py:57-102): input_proj 1x1 1024->256 + bias straight over xs16
  // -> src [B*T, 256] and its scale slot, unless the last block's tail already wrote src
  if (!x.src_ready) {
    GemmArgs g = linear_args(m->inproj, f.P(x.x), x.ld, f.Mt, f.P(w.src), f.d);
    g.amax_a = x.amax; g.amax_c = f.slot(SPE_AMAX_BB - 1);
    CK(run_gemm(m, "gemm.input_proj", g, GEMM_LINEAR, s));
  }
  return 0;
}

// ---------------- encoder (REV/models/transformer.py:154-167)

struct EncAttn {             // operand forms of the encoder attention, the same for every layer
  int f16attn, f16v, attn_dt, vt_swz, split_swz, split_f16;
  bool presplit;
};

EncAttn enc_attn_forms(const Fwd& f) {
  const spe_model* m = f.m;
  const auto& c = m->cfg;
  const int dt = f.dt, T = f.T;
  EncAttn a{};
  // fp16 encoder attention operands (bf16 models, attn_dtype = SPE_DTYPE_F16_): the q/k and V^T
  // projections store fp16, the attention runs fp16 MFMAs; everything else stays bf16
  a.f16attn = c.attn_dtype == SPE_DTYPE_F16_ && dt == SPE_DTYPE_BF16;
  // bf16 models otherwise keep bf16 q/k but store V^T as fp16: the attention's P is then fp16
  // and its row sums packed-fp16 adds (attention.hip, TV).  fp16 has the finer mantissa; V and
  // P stay far inside its range.  SPE_ATTN_F16V=0 keeps V^T and P bf16 (A/B knob).
  static const int f16v_env = spe_env_int("SPE_ATTN_F16V", 1);
  a.f16v = !a.f16attn && dt == SPE_DTYPE_BF16 && f16v_env;
  a.attn_dt = a.f16attn ? SPE_DTYPE_F16 : a.f16v ? SPE_DTYPE_BF16_F16V : dt;
  // 16-bit encoder attention stages K / V^T by LDS DMA, which needs V^T rows in its key order
  // (vt_pos: the v projection's epilogue writes them so); SPE_ATTN_DMA=0 keeps register staging
  static const int dma_env = spe_env_int("SPE_ATTN_DMA", 1);
  a.vt_swz = dma_env && dt == SPE_DTYPE_BF16 && T % 16 == 0;
  // fp32x3 / fp32x6 encoder attention: the q/k and v projection epilogues write K and V^T as bf16
  // hi / lo planes (GemmArgs::S) that the attention stages as plain copies (SPE_ATTN_PRESPLIT=0:
  // fp32 K / V^T, split per tile inside the attention)
  static const int ps_env = spe_env_int("SPE_ATTN_PRESPLIT", 1);
  a.presplit = ps_env && f.w.kpl && x3_for(m, "attn.enc") && T % 8 == 0;
  // ... with V^T in the 16-bit key order (T % 16 == 0): the LDS-DMA split kernel (attn_split.hip); the
  // fp32h3 model's V^T planes are then fp16 of V * 2^-ev, ev from max |src| . max_n |Wv[n]|_1 + max |bv|
  a.split_swz = a.presplit && T % 16 == 0;
  a.split_f16 = a.split_swz && m->h3 && f.amx;
  return a;
}

// q/k and V^T projections + self-attention of x (src; a pre-norm model's norm1(src)) into ao; the attention
// output's scale slot is o_amax
int enc_self_attention(Fwd& f, const Enc& e, const EncAttn& ea, const void* x, const float* src_amax, float* o_amax) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  hipStream_t s = f.s;
  const int B = f.B, T = f.T, d = f.d, Mt = f.Mt;
  {
    GemmArgs g = linear_args(e.qk, x, d, Mt, f.P(w.qkv), 3 * d);
    g.out_f16 = ea.f16attn;
    g.amax_a = src_amax;
    if (ea.presplit) { g.S = f.P(w.kpl); g.s_col0 = d; }
    const int mode = add_pos(m, g, m->pos, d, T, e.pos_qk, 2 * d);
    CK(run_gemm(m, "gemm.enc.qk", g, mode, s));
  }
  {
    GemmArgs g = linear_args(e.v, x, d, Mt, f.P(w.vt), 8);
    g.vt_T = T; g.vt_B = B; g.vt_swz = ea.vt_swz;
    // the attention output is a convex combination of V rows: max |V| bounds it
    g.amax_a = src_amax; g.amax_c = o_amax;
    g.out_f16 = ea.f16attn || ea.f16v;
    if (ea.presplit) g.S = f.P(w.vt);            // hi plane then lo plane, in the fp32 V^T's bytes
    if (ea.split_swz) g.vt_swz = 1;
    if (ea.split_f16) { g.s_f16 = 1; g.s_l1 = e.v.l1max; g.s_bmax = e.v.bmax; }
    CK(run_gemm(m, "gemm.enc.v", g, GEMM_LINEAR, s));
  }
  AttnArgs a{};
  a.q = f.P(w.qkv); a.ldq = 3 * d;
  a.k = ea.presplit ? f.P(w.kpl) : (char*)f.P(w.qkv) + d * m->esz; a.ldk = ea.presplit ? d : 3 * d;
  a.presplit = ea.presplit;
  a.vt = f.P(w.vt); a.vt_swz = ea.vt_swz || ea.split_swz;
  if (ea.split_f16) { a.v_f16 = 1; a.v_amax = src_amax; a.v_l1 = e.v.l1max; a.v_bmax = e.v.bmax; }
  a.o = f.P(w.ao); a.ldo = d;
  a.B = B; a.H = m->cfg.nheads; a.Tq = T; a.Tk = T; a.scale = f.scale;
  CK(run_attn(m, "attn.enc", a, ea.attn_dt, s));
  return 0;
}

// spe_forward_attention: the map of the self-attention whose q / k enc_self_attention left in qkv (the
// operands its attention kernel read: bf16, fp16 with attn_dtype fp16, or fp32)
int enc_attn_map(Fwd& f, const EncAttn& ea, float* map) {
  spe_model* m = f.m;
  const int d = f.d, T = f.T;
  AttnMapArgs a{};
  a.q = f.P(f.w.qkv); a.q_sb = (long long)T * 3 * d; a.q_sh = 32; a.ldq = 3 * d;
  a.k = (char*)f.P(f.w.qkv) + d * m->esz; a.k_sb = a.q_sb; a.k_sh = 32; a.ldk = 3 * d;
  a.out = map;
  a.B = f.B; a.H = m->cfg.nheads; a.Tq = T; a.Tk = T; a.head_dim = 32; a.scale = f.scale;
  const double fl = 2.0 * 2.0 * f.B * 8.0 * T * (double)T * 32;
  const double by = (double)f.B * T * (double)T * 4 + 2.0 * f.Mt * d * m->esz;
  const int dt = ea.f16attn ? SPE_DTYPE_F16 : f.dt;
  CK(run_other(m, "attn.map", fl, by, f.s, [&] { return spe_launch_attn_map(a, dt, f.s); }));
  return 0;
}

// encoder layer li over src (in place); *src_amax: the scale input of src, before and after
int encoder_layer(Fwd& f, const Enc& e, int li, const EncAttn& ea, const float** src_amax) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  hipStream_t s = f.s;
  const int d = f.d, ff = f.ff, Mt = f.Mt;
  float* const o_amax = f.slot(SPE_AMAX_BB + 2 * li);
  TRY(enc_self_attention(f, e, ea, f.P(w.src), *src_amax, o_amax));
  if (f.tap && f.tap->enc_map && f.tap->enc_layer == li) TRY(enc_attn_map(f, ea, f.tap->enc_map));
  {
    // out-proj + residual; bf16 large batches fuse norm1 into the GEMM epilogue, in place over src
    GemmArgs gf = linear_args(e.o, f.P(w.ao), d, Mt, f.P(w.src), d);
    gf.R = f.P(w.src); gf.ldr = d;
    gf.amax_a = o_amax;
    gf.ln_g = e.n1g; gf.ln_b = e.n1b;
    // (fp32h3 runs the persistent GEMM + the LayerNorm kernel: 0.15 + 0.06 ms a layer against 0.31 ms
    // for the fused 256-wide h3 tile with a LayerNorm epilogue, which ended every tile cold; removed)
    if (m->esz == 2 && spe_ln_fusable(gf))
      CK(run_gemm(m, "gemm.enc.o", gf, GEMM_LINEAR, s));
    else
      TRY(linear_residual_ln(f, "gemm.enc.o", "ln.enc", e.o, f.P(w.ao), d, o_amax, Mt, f.P(w.src), f.P(w.tmp), e.n1g,
                             e.n1b));
    *src_amax = e.n1_bound;
  }
  if (use_fused_ffn(m)) {
    // the last layer also emits memory + pos for the cross-K projection (xattn adds pos itself)
    const bool last = &e == &m->enc.back();
    CK(run_ffn(m, "ffn.enc", e.l1, e.l2, e.n2g, e.n2b, f.P(w.src), Mt, s, last ? m->pos : nullptr,
               last ? f.P(w.srcpos) : nullptr, f.T, nullptr, e.ffn_w2c));
  } else if (m->h3 && e.ffn_w2p && *src_amax && m->wh3.count(e.l1.w)) {
    // fp32h3: linear1 + ReLU + linear2 + residual + norm2 in one pass, in place over src
    FfnH3Args a{};
    a.x = (const float*)f.P(w.src); a.ldx = d; a.y = (float*)f.P(w.src); a.ldy = d;
    a.M = Mt; a.D = d; a.F = ff;
    a.w1 = m->wh3.at(e.l1.w).planes; a.ld1 = e.l1.Kpad; a.meta1 = e.ffn_meta1;
    a.w2 = e.ffn_w2p; a.ld2 = ff; a.sinv2 = m->wh3.at(e.l2.w).sinv; a.b2 = e.l2.bias;
    a.gamma = e.n2g; a.beta = e.n2b;
    a.amax_x = *src_amax; a.sh = e.ffn_sh;
    const double fl = 4.0 * Mt * (double)d * ff, by = 2.0 * Mt * d * 4.0 + 2.0 * 2.0 * 2.0 * d * ff;
    CK(ledger_use(a.amax_x, nullptr, "ffn.enc"));
    CK(run_other(m, "ffn.enc", fl, by, s, [&] { return spe_launch_ffn_h3(a, s); }));
  } else {
    // (fp32h3 likewise: the persistent GEMM + LayerNorm, 0.65 + 0.06 against 0.85 ms fused)
    TRY(unfused_ffn(f, "gemm.enc.ffn1", "gemm.enc.ffn2", "ln.enc", e.l1, e.l2, f.P(w.src), *src_amax, Mt, f.P(w.ffn),
                    f.slot(SPE_AMAX_BB + 2 * li + 1), f.P(w.tmp), e.n2g, e.n2b));
  }
  *src_amax = e.n2_bound;
  return 0;
}

// ---------------- pre-norm encoder (REV/models/transformer.py forward_pre, TransformerEncoder.forward)
//
// The residual stream s lives in src (the backbone writes it there); its normed copy n lives in nrm.  Per layer
//     n = norm1(s); q = k = n + pos; s += out_proj(attn(q, k, n)); s += linear2(relu(linear1(norm2(s))))
// and after the last layer memory = encoder.norm(s), again in nrm: every reader of the memory (the cross K / V
// projections, xattn.hip) takes nrm in a pre-norm model where it takes src in a post-norm one.
//   bf16: per layer the post-norm model's five kinds -- gemm.enc.qk, gemm.enc.v, attn.enc, gemm.enc.o (lnproj.hip's
//         form without the LayerNorm, in place over s) and ffn.enc (ffn.hip's pre form: norm2 on chip, and the NEXT
//         consumer's LayerNorm -- the next layer's norm1 or encoder.norm -- stored beside s, so only layer 0's norm1
//         is a launch of its own, one ln.enc in front).
//   fp32 modes: GEMM + LayerNorm launches; the out-projection writes s into tmp, linear2 back into src.
int encoder_layer_pre(Fwd& f, const Enc& e, int li, const EncAttn& ea) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  hipStream_t s = f.s;
  const int d = f.d, Mt = f.Mt;
  const bool last = &e == &m->enc.back();
  const float* ng = last ? m->eng : m->enc[li + 1].n1g;   // the LayerNorm the next reader of s applies
  const float* nb = last ? m->enb : m->enc[li + 1].n1b;
  TRY(enc_self_attention(f, e, ea, f.P(w.nrm), nullptr, nullptr));
  if (f.tap && f.tap->enc_map && f.tap->enc_layer == li) TRY(enc_attn_map(f, ea, f.tap->enc_map));
  size_t cur = w.src;
  {
    GemmArgs g = linear_args(e.o, f.P(w.ao), d, Mt, f.P(w.src), d);
    g.R = f.P(w.src); g.ldr = d;
    if (m->esz == 2 && spe_lnproj_pre_applies(g)) {
      const double by = ((double)Mt * d * 3 + (double)d * d) * m->esz;
      CK(run_other(m, "gemm.enc.o", 2.0 * Mt * d * d, by, s, [&] { return spe_launch_lnproj_pre(g, s); }));
    } else {
      g.C = f.P(w.tmp);
      CK(run_gemm(m, "gemm.enc.o", g, GEMM_LINEAR, s));
      cur = w.tmp;
    }
  }
  if (use_fused_ffn(m)) {
    CK(run_ffn_pre(m, "ffn.enc", e.l1, e.l2, e.n2g, e.n2b, f.P(cur), f.P(w.src), ng, nb, f.P(w.nrm), Mt, s,
                   last ? m->pos : nullptr, last ? f.P(w.srcpos) : nullptr, f.T, nullptr, e.ffn_w2c));
    return 0;
  }
  CK(run_layernorm(m, "ln.enc", f.P(cur), e.n2g, e.n2b, f.P(w.nrm), nullptr, Mt, d, f.dt, s));
  {
    GemmArgs g = linear_args(e.l1, f.P(w.nrm), d, Mt, f.P(w.ffn), f.ff);
    g.act = ACT_RELU;
    CK(run_gemm(m, "gemm.enc.ffn1", g, GEMM_LINEAR, s));
  }
  {
    // (cur is tmp here: only a bf16 model takes the in-place out-projection, and every bf16 model the fused FFN)
    GemmArgs g = linear_args(e.l2, f.P(w.ffn), f.ff, Mt, f.P(w.src), d);
    g.R = f.P(cur); g.ldr = d;
    CK(run_gemm(m, "gemm.enc.ffn2", g, GEMM_LINEAR, s));
  }
  CK(run_layernorm(m, "ln.enc", f.P(w.src), ng, nb, f.P(w.nrm), nullptr, Mt, d, f.dt, s));
  return 0;
}

// The tail of both encoder stages unless the decoder attends to the memory itself (xattn): all decoder layers'
// cross-attention K (memory + pos) and V^T (memory) from `mem` (src; a pre-norm model's nrm) into ck / cvt.
// mem_amax: mem's fp32h3 scale input; v_amax: the slot the V^T GEMM raises, bounding every cross-attention output
int cross_kv_projection(Fwd& f, const void* mem, const float* mem_amax, float* v_amax) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  const int T = f.T, d = f.d, L = f.L, Mt = f.Mt;
  {
    // bf16 fused path: the last FFN wrote memory + pos (rounded once, like the reference's
    // fp32 add) -> plain GEMM; its 8 MB pos.W^T table would not stay L2-resident
    const bool have_srcpos = use_fused_ffn(m) && !m->enc.empty();
    GemmArgs g = linear_args(m->crossK, have_srcpos ? f.P(w.srcpos) : mem, d, Mt, f.P(w.ck), L * d);
    const int mode = have_srcpos ? GEMM_LINEAR : add_pos(m, g, m->pos, d, T, m->pos_crossK, L * d);
    if (!have_srcpos) g.amax_a = mem_amax;
    CK(run_gemm(m, "gemm.cross_kv", g, mode, f.s));
  }
  GemmArgs g = linear_args(m->crossV, mem, d, Mt, f.P(w.cvt), 8);
  g.vt_T = T; g.vt_B = f.B;
  g.amax_a = mem_amax; g.amax_c = v_amax;
  CK(run_gemm(m, "gemm.cross_kv", g, GEMM_LINEAR, f.s));
  return 0;
}

int encoder_stage_pre(Fwd& f) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  hipStream_t s = f.s;
  const int d = f.d, Mt = f.Mt;
  const EncAttn ea = enc_attn_forms(f);
  // layer 0's norm1(src); without encoder layers the memory is encoder.norm(src)
  CK(run_layernorm(m, "ln.enc", f.P(w.src), m->enc.empty() ? m->eng : m->enc[0].n1g,
                   m->enc.empty() ? m->enb : m->enc[0].n1b, f.P(w.nrm), nullptr, Mt, d, f.dt, s));
  int li = 0;
  for (const Enc& e : m->enc) TRY(encoder_layer_pre(f, e, li++, ea));
  if (spe_use_xattn(m)) return 0;               // (bf16: the last FFN wrote memory + pos into srcpos)
  return cross_kv_projection(f, f.P(w.nrm), nullptr, nullptr);
}

int encoder_stage(Fwd& f) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  hipStream_t s = f.s;
  const int B = f.B, T = f.T, d = f.d, Mt = f.Mt;
  TRY(zero_slots(f, SPE_AMAX_BB, SPE_AMAX_DEC - SPE_AMAX_BB));
  const float* src_amax = f.slot(SPE_AMAX_BB - 1);
  const EncAttn ea = enc_attn_forms(f);
  int li = 0;
  for (const Enc& e : m->enc) TRY(encoder_layer(f, e, li++, ea, &src_amax));
  // memory = src.  Unless the layers attend to memory + pos / memory directly (xattn path),
  // project the cross-attention K (memory + pos) and V^T (memory) for all decoder layers.
  if (spe_use_xattn(m)) {
    if (!m->h3) return 0;
    // fp32h3: the memory once as fp16 planes for all decoder layers (xattn_h3.hip): key planes of
    // memory + pos into srcpos, value planes into xvp
    CK(ledger_use(src_amax, nullptr, "eltwise.xsplit"));
    CK(run_other(m, "eltwise.xsplit", 0.0, (double)Mt * d * (4 + 4 + 4) + (double)T * d * 4, s, [&] {
      return spe_launch_xattn_h3_split((const float*)f.P(w.src), (const float*)m->pos, src_amax, f.P(w.srcpos),
                                       f.P(w.xvp), B, T, s);
    }));
    return 0;
  }
  return cross_kv_projection(f, f.P(w.src), src_amax, f.slot(SPE_AMAX_DEC - 1));
}

// ---------------- decoder (REV/models/transformer.py:100-129,218-239)

// A/B knobs of the bf16 decoder kernels (decsa.hip), each read once
// SPE_DECPROJ=0: the out-projection + LayerNorm (and the cross-attention tail) as GEMM + LayerNorm launches
bool decproj_on() {
  static const bool on = spe_env_int("SPE_DECPROJ", 1) != 0;
  return on;
}
// bf16: the decoder FFN and the cross-attention's query projection as decsa.hip's 16-row kernels;
// SPE_DECFFN=0 runs ffn.hip's FFN and the GEMM for A/B runs
bool decffn_on() {
  static const bool on = spe_env_int("SPE_DECFFN", 1) != 0;
  return on;
}

// tgt = LayerNorm(tgt + dao . W^T + b) (REV/models/transformer.py:227-228, 233-234) as GEMM +
// LayerNorm: at these few rows (B.Q) lnproj's one-workgroup-per-8-tiles form measured slower
// (24 vs 18 us a layer: 6 workgroups each staging all of W)
int dec_proj_ln(Fwd& f, const Conv& wo, const void* fwo, const float* lg, const float* lb, const float* x_amax) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  const int d = f.d, Mq = f.Mq;
  if (decproj_on() && fwo && f.Q <= 64) {
    // bf16: one workgroup per image, the rows in LDS from the GEMM to the LayerNorm (decsa.hip)
    DecProjArgs pa{};
    pa.tgt = f.P(w.tgt); pa.ldt = d; pa.x = f.P(w.dao); pa.ldx = d; pa.B = f.B; pa.Q = f.Q;
    pa.wo = fwo; pa.bo = wo.bias; pa.g = lg; pa.b = lb;
    CK(run_other(m, "dec.proj", 2.0 * Mq * d * d, 3.0 * Mq * d * m->esz + (double)d * d * m->esz, f.s,
                 [&] { return spe_launch_decproj(pa, f.s); }));
    return 0;
  }
  return linear_residual_ln(f, "gemm.dec", "ln.dec", wo, f.P(w.dao), d, x_amax, Mq, f.P(w.tgt), f.P(w.dtmp), lg, lb);
}

// q/k (x + query_pos) and V^T projections + self-attention of the rows x (tgt; a pre-norm model's norm1(t)) into
// dao; x_amax: x's fp32h3 scale input, o_amax: the slot the V^T projection raises, which bounds the attention output
int dec_self_attention(Fwd& f, const Dec& e, const void* x, const float* x_amax, float* o_amax) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  hipStream_t s = f.s;
  const int B = f.B, Q = f.Q, d = f.d, Mq = f.Mq;
  {
    GemmArgs g = linear_args(e.sqk, x, d, Mq, f.P(w.dqkv), 3 * d);
    const int mode = add_pos(m, g, m->qpos, d, Q, e.qpos_sqk, 2 * d);
    g.amax_a = x_amax;
    CK(run_gemm(m, "gemm.dec", g, mode, s));
  }
  {
    GemmArgs g = linear_args(e.sv, x, d, Mq, f.P(w.dvt), 8);
    g.vt_T = Q; g.vt_B = B;
    g.amax_a = x_amax; g.amax_c = o_amax;
    CK(run_gemm(m, "gemm.dec", g, GEMM_LINEAR, s));
  }
  AttnArgs a{};
  a.q = f.P(w.dqkv); a.ldq = 3 * d;
  a.k = (char*)f.P(w.dqkv) + d * m->esz; a.ldk = 3 * d;
  a.vt = f.P(w.dvt);
  a.o = f.P(w.dao); a.ldo = d;
  a.B = B; a.H = m->cfg.nheads; a.Tq = Q; a.Tk = Q; a.scale = f.scale;
  CK(run_attn(m, "attn.dec_self", a, f.dt, s));
  return 0;
}

// self-attention block of layer l: projections, attention, out-projection, norm1 over tgt
int dec_self_block(Fwd& f, const Dec& e, int l, const float* tgt_amax) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  hipStream_t s = f.s;
  const int B = f.B, Q = f.Q, d = f.d, Mq = f.Mq;
  // bf16: the self-attention block (projections, attention, out-projection, norm1) as one
  // launch per layer (decsa.hip); SPE_DECSA=0 runs the separate launches for A/B runs
  static const bool decsa_on = spe_env_int("SPE_DECSA", 1) != 0;
  if (decsa_on && e.fsqk && m->cfg.nheads == 8 && Q <= 64 && e.qpos_sqk) {
    DecSaArgs sa{};
    sa.tgt = f.P(w.tgt); sa.ldt = d; sa.B = B; sa.Q = Q;
    sa.wqk = e.fsqk; sa.bqk = e.sqk.bias;
    sa.wv = e.fsv; sa.bv = e.sv.bias;
    sa.qpos = e.qpos_sqk;
    sa.wo = e.fso; sa.bo = e.so.bias;
    sa.g = e.n1g; sa.b = e.n1b; sa.scale = f.scale;
    const double fl = 2.0 * Mq * d * (4.0 * d) + 4.0 * B * 8.0 * Q * Q * 32;
    const double by = 2.0 * Mq * d * m->esz + 4.0 * d * d * m->esz;
    CK(run_other(m, "dec.self", fl, by, s, [&] { return spe_launch_decsa(sa, s); }));
    return 0;
  }
  float* const o_amax = f.slot(SPE_AMAX_DEC + 2 * l);   // the sv GEMM's published maximum
  TRY(dec_self_attention(f, e, f.P(w.tgt), tgt_amax, o_amax));
  return dec_proj_ln(f, e.so, e.fso, e.n1g, e.n1b, o_amax);
}

// cross-attention against the memory itself (xattn.hip / xattn_h3.hip): q' rows against the key operand
// k and the value operand v
XattnArgs xattn_args(const Fwd& f, const Dec& e, const void* k, int ldk, const void* v, int ldv) {
  const Ws& w = f.w;
  XattnArgs x{};
  x.q = f.P(w.xq); x.ldq = 8 * f.d;
  x.k = k; x.ldk = ldk;
  x.v = v; x.ldv = ldv;
  x.wv = e.xv.w; x.bv = e.xv.bias;
  x.o = f.P(w.dao); x.ldo = f.d;
  x.B = f.B; x.Q = f.Q; x.T = f.T; x.splits = spe_xattn_splits(f.B, f.Q, f.T);
  x.pm = (float*)f.P(w.xpm); x.pl = (float*)f.P(w.xpl); x.pu = (float*)f.P(w.xpu);
  return x;
}

// q' = (x + query_pos) . Wqk^T + bqk into xq: the query-side fold of Wq and Wk (xattn.hip) over the rows x (tgt; a
// pre-norm model's norm2(t)); x_amax: the h3 GEMM's scale input (fp32h3)
int dec_cross_query(Fwd& f, const Dec& e, const void* x, const float* x_amax) {
  spe_model* m = f.m;
  hipStream_t s = f.s;
  const int Q = f.Q, d = f.d, Mq = f.Mq;
  if (e.fxq && decffn_on()) {
    // (16 rows, 256 columns) workgroups over the packed weights (decsa.hip)
    DecQArgs qa{};
    qa.x = x; qa.ldx = d; qa.M = Mq; qa.N = 8 * d;
    qa.w = e.fxq; qa.bias = e.xq.bias; qa.R = e.xq_r; qa.ldr = 8 * d; qa.period = Q;
    qa.y = f.P(f.w.xq); qa.ldy = 8 * d;
    CK(run_other(m, "gemm.dec", 2.0 * Mq * d * 8.0 * d, 2.0 * Mq * (d + 8.0 * d) * m->esz + 2.0 * 8 * d * d * m->esz, s,
                 [&] { return spe_launch_decq(qa, s); }));
    return 0;
  }
  GemmArgs g = linear_args(e.xq, x, d, Mq, f.P(f.w.xq), 8 * d);
  g.R = e.xq_r; g.ldr = 8 * d; g.r_period = Q;
  g.amax_a = x_amax;
  CK(run_gemm(m, "gemm.dec", g, GEMM_LINEAR, s));
  return 0;
}

// cross-attention of layer l against the memory (spe_use_xattn) into dao, or straight through the
// out-projection + norm2 into tgt (*xtail); *o_amax: the out-projection's fp32h3 scale input
int dec_xattn(Fwd& f, const Dec& e, int l, const float* tgt_amax, const float** o_amax, bool* xtail) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  hipStream_t s = f.s;
  const int B = f.B, Q = f.Q, T = f.T, d = f.d, L = f.L, Mq = f.Mq;
  TRY(dec_cross_query(f, e, f.P(w.tgt), tgt_amax));
  if (m->h3) {
    // fp32h3: scores and value sums against the memory's fp16 planes, three products each; the
    // merge applies Wv / bv in fp32 and raises max |o| for the out-projection
    XattnArgs x = xattn_args(f, e, f.P(w.srcpos), 2 * d, f.P(w.xvp), 2 * d);
    // the memory's bound (the last encoder norm2's) scales its planes; layer l's output raises slot
    // SPE_AMAX_DEC + 2L + l
    x.mem_amax = m->enc.empty() ? nullptr : m->enc.back().n2_bound;
    x.o_amax = f.slot(SPE_AMAX_DEC + 2 * L + l);
    const double fl = 4.0 * B * 8.0 * Q * (double)T * d + 2.0 * Mq * 8.0 * d * 32;
    const double by = 2.0 * B * (double)T * 2 * d * 2 + 2.0 * Mq * 8.0 * d * 4;
    CK(ledger_use(x.mem_amax, x.o_amax, "attn.dec_cross"));
    CK(run_other(m, "attn.dec_cross", fl, by, s, [&] { return spe_launch_xattn_h3(x, s); }));
    *o_amax = x.o_amax;
    return 0;
  }
  XattnArgs x = xattn_args(f, e, f.P(w.srcpos), d, f.P(w.src), d);
  // Q <= 48: the split merge and the value projection move into the out-projection + norm2
  // launch (decsa.hip decxproj_kernel), the per-split partials its only input
  *xtail = decproj_on() && e.fxv && Q <= 48;
  x.partials_only = *xtail;
  const double fl = 4.0 * B * 8.0 * Q * (double)T * d + (*xtail ? 0.0 : 2.0 * Mq * 8.0 * d * 32);
  const double by = 2.0 * B * (double)T * d * m->esz + 2.0 * Mq * 8.0 * d * m->esz;
  CK(run_other(m, "attn.dec_cross", fl, by, s, [&] { return spe_launch_xattn(x, s); }));
  if (!*xtail) return 0;
  DecProjArgs pa{};
  pa.tgt = f.P(w.tgt); pa.ldt = d; pa.B = B; pa.Q = Q;
  pa.wo = e.fco; pa.bo = e.co.bias; pa.g = e.n2g; pa.b = e.n2b;
  pa.pm = x.pm; pa.pl = x.pl; pa.pu = x.pu; pa.splits = spe_xattn_launch_splits(T, x.splits);
  pa.wv = e.fxv; pa.bv = e.xv.bias;
  const double pfl = 2.0 * Mq * 8.0 * d * 32 + 2.0 * Mq * d * d;
  const double pby = (double)pa.splits * B * 8.0 * Q * (d + 2) * 4 + 2.0 * Mq * d * m->esz + 2.0 * d * d * m->esz;
  CK(run_other(m, "dec.xproj", pfl, pby, s, [&] { return spe_launch_decproj(pa, s); }));
  return 0;
}

// spe_forward_attention: the map of layer l's cross-attention from the operands its attention kernel
// read.  Against the memory (bf16, xattn.hip): the folded q' [B*Q][8*256] in xq, already in the exp2
// domain, and memory + pos in srcpos as every head's key.  Else the projected q in dqc and layer l's
// slice of the projected keys ck.
int dec_attn_map(Fwd& f, int l, float* map) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  const int Q = f.Q, T = f.T, d = f.d, L = f.L;
  AttnMapArgs a{};
  a.out = map;
  a.B = f.B; a.H = m->cfg.nheads; a.Tq = Q; a.Tk = T;
  if (spe_use_xattn(m)) {
    a.q = f.P(w.xq); a.q_sb = (long long)Q * 8 * d; a.q_sh = d; a.ldq = 8 * d;
    a.k = f.P(w.srcpos); a.k_sb = (long long)T * d; a.k_sh = 0; a.ldk = d;
    a.head_dim = d; a.base2 = 1; a.scale = 1.f;
  } else {
    a.q = f.P(w.dqc); a.q_sb = (long long)Q * d; a.q_sh = 32; a.ldq = d;
    a.k = (char*)f.P(w.ck) + (size_t)l * d * m->esz; a.k_sb = (long long)T * L * d; a.k_sh = 32; a.ldk = L * d;
    a.head_dim = 32; a.scale = f.scale;
  }
  const double fl = 2.0 * 2.0 * f.B * 8.0 * Q * (double)T * a.head_dim;
  const double by = (double)f.B * Q * (double)T * 4 + (double)f.Mt * d * m->esz;
  CK(run_other(m, "attn.map", fl, by, f.s, [&] { return spe_launch_attn_map(a, f.dt, f.s); }));
  return 0;
}

// cross-attention of layer l against the memory's projected K / V^T (layer l's slices of ck / cvt) into dao: the
// query projection of the rows x + query_pos (tgt; a pre-norm model's norm2(t)) into dqc, then the attention
int dec_cross_attention_projected(Fwd& f, const Dec& e, int l, const void* x, const float* x_amax) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  const int B = f.B, Q = f.Q, T = f.T, d = f.d, L = f.L;
  GemmArgs g = linear_args(e.cq, x, d, f.Mq, f.P(w.dqc), d);
  const int mode = add_pos(m, g, m->qpos, d, Q, e.qpos_cq, d);
  g.amax_a = x_amax;
  CK(run_gemm(m, "gemm.dec", g, mode, f.s));
  AttnArgs a{};
  a.q = f.P(w.dqc); a.ldq = d;
  a.k = (char*)f.P(w.ck) + (size_t)l * d * m->esz; a.ldk = L * d;
  a.vt = (char*)f.P(w.cvt) + (size_t)l * B * d * T * m->esz;
  a.o = f.P(w.dao); a.ldo = d;
  a.B = B; a.H = m->cfg.nheads; a.Tq = Q; a.Tk = T; a.scale = f.scale;
  CK(run_attn(m, "attn.dec_cross", a, f.dt, f.s));
  return 0;
}

// cross-attention block of layer l: attention against the memory or its projected K / V^T (ck / cvt),
// out-projection, norm2 over tgt
int dec_cross_block(Fwd& f, const Dec& e, int l, const float* tgt_amax) {
  spe_model* m = f.m;
  bool xtail = false;                         // the merge + value + out-projection + norm2 ran in one launch
  // fp32h3: the out-projection's scale input (the crossV GEMM's published maximum, transformer stage)
  const float* cross_o_amax = f.slot(SPE_AMAX_DEC - 1);
  if (spe_use_xattn(m)) {
    TRY(dec_xattn(f, e, l, tgt_amax, &cross_o_amax, &xtail));
  } else {
    TRY(dec_cross_attention_projected(f, e, l, f.P(f.w.tgt), tgt_amax));
  }
  if (f.tap && f.tap->dec_map && f.tap->dec_layer == l) TRY(dec_attn_map(f, l, f.tap->dec_map));
  if (!xtail) TRY(dec_proj_ln(f, e.co, e.fco, e.n2g, e.n2b, cross_o_amax));
  return 0;
}

// FFN block of layer l: linear1, ReLU, linear2, norm3 over tgt
int dec_ffn_block(Fwd& f, const Dec& e, int l, const float* tgt_amax) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  hipStream_t s = f.s;
  const int d = f.d, ff = f.ff, Mq = f.Mq;
  if (e.fl1 && decffn_on()) {
    // bf16: one workgroup per (16 rows, 256 hidden units), all of its weight fragments in flight
    // from the start (decsa.hip), then ffn.hip's split-F reduce + norm3
    DecFfnArgs fa{};
    fa.x = f.P(w.tgt); fa.ldx = d; fa.M = Mq; fa.F = ff;
    fa.w1 = e.fl1; fa.b1 = e.l1.bias; fa.w2 = e.fl2; fa.partial = (float*)f.P(w.dffnpart);
    FfnArgs ra{};
    ra.x = f.P(w.tgt); ra.ldx = d; ra.y = f.P(w.tgt); ra.ldy = d; ra.M = Mq; ra.D = d; ra.F = ff;
    ra.b2 = e.l2.bias; ra.gamma = e.n3g; ra.beta = e.n3b; ra.splits = ff / 256; ra.partial = fa.partial;
    const double fl = 4.0 * Mq * (double)d * ff;
    const double by = 2.0 * Mq * d * m->esz + 2.0 * (double)d * ff * m->esz + 2.0 * ra.splits * Mq * d * 4;
    CK(run_other(m, "ffn.dec", fl, by, s, [&] {
      const int rc = spe_launch_decffn(fa, s);
      return rc ? rc : spe_launch_ffn_reduce_ln(ra, s);
    }));
    return 0;
  }
  if (use_fused_ffn(m)) {
    CK(run_ffn(m, "ffn.dec", e.l1, e.l2, e.n3g, e.n3b, f.P(w.tgt), Mq, s, nullptr, nullptr, 0,
               (float*)f.P(w.dffnpart)));
    return 0;
  }
  return unfused_ffn(f, "gemm.dec", "gemm.dec", "ln.dec", e.l1, e.l2, f.P(w.tgt), tgt_amax, Mq, f.P(w.dffn),
                     f.slot(SPE_AMAX_DEC + 2 * l + 1), f.P(w.dtmp), e.n3g, e.n3b);
}

// the shared decoder_norm (REV/models/transformer.py:117-124) of tgt into hs, then the heads
// (REV/models/detr_speed.py:83-99); the final call also runs the sigma head and the fused PostProcess
// (REV/models/detr_speed.py:83-92,266-293), an aux layer's writes logits and points only
int run_heads(Fwd& f, const void* tgt, float* hs, float* logits, float* points, bool final,
              const spe_forward_outputs& out) {
  spe_model* m = f.m;
  CK(run_layernorm(m, "ln.dec", tgt, m->dng, m->dnb, nullptr, hs, f.Mq, f.d, f.dt, f.s));
  HeadArgs h = m->head;
  h.hs = hs; h.B = f.B; h.Q = f.Q;
  h.logits = logits; h.points = points;
  const bool px = final && out.clip_bbox, sigma = final && m->cfg.sigma_head;
  h.clip_bbox = final ? out.clip_bbox : nullptr;
  h.probs = px ? out.probs : nullptr;
  h.points_px = px ? out.points_px : nullptr;
  h.log_sigmas = sigma ? out.log_sigmas : nullptr;
  h.sigmas = sigma ? out.sigmas : nullptr;
  CK(run_other(m, "heads", 0.0, (double)f.Mq * f.d * 4, f.s, [&] { return spe_launch_heads(h, f.s); }));
  return 0;
}

// the aux output of decoder layer l (every layer but the last, when the call asks for aux outputs): the heads
// over the layer's output rows tgt, into layer l's slices of the aux outputs
int aux_heads(Fwd& f, int l, const void* tgt, const spe_forward_outputs& out) {
  if (!out.aux_logits || !out.aux_points || l + 1 >= f.L) return 0;
  return run_heads(f, tgt, (float*)f.P(f.w.hs), out.aux_logits + (size_t)l * f.Mq * 12,
                   out.aux_points + (size_t)l * f.Mq * 2, false, out);
}

// (reads only the memory -- src, srcpos, or ck / cvt -- that the encode stage left in the
// workspace, so the two stages may run on different streams, e.g. batch i's decoder beside
// batch i+1's backbone with two workspaces)
int decoder_stage(Fwd& f, const spe_forward_outputs& out) {
  spe_model* m = f.m;
  const int L = f.L, Mq = f.Mq;
  CK((int)hipMemsetAsync(f.P(f.w.tgt), 0, (size_t)Mq * f.d * m->esz, f.s));
  // fp32h3 decoder scales: tgt's from its LayerNorm bounds (zeros before the first layer: any scale
  // serves), the attention outputs' from their V (self: the sv GEMM's published maximum; cross: the
  // crossV GEMM's, transformer stage), the FFN hidden's from the linear1 GEMM
  TRY(zero_slots(f, SPE_AMAX_DEC, SPE_AMAX_SLOTS - SPE_AMAX_DEC));
  const float* tgt_amax = m->h3 && L > 0 ? m->dec[0].n1_bound : nullptr;
  for (int l = 0; l < L; ++l) {
    const Dec& e = m->dec[l];
    TRY(dec_self_block(f, e, l, tgt_amax));
    if (m->h3) tgt_amax = e.n1_bound;
    TRY(dec_cross_block(f, e, l, tgt_amax));
    if (m->h3) tgt_amax = e.n2_bound;
    TRY(dec_ffn_block(f, e, l, tgt_amax));
    if (m->h3) tgt_amax = e.n3_bound;
    TRY(aux_heads(f, l, f.P(f.w.tgt), out));
  }
  CK(run_heads(f, f.P(f.w.tgt), out.hs ? out.hs : (float*)f.P(f.w.hs), out.logits, out.points, true, out));
  return 0;
}

// ---------------- pre-norm decoder (REV/models/transformer.py forward_pre of TransformerDecoderLayer)
//
//     n = norm1(t); q = k = n + query_pos; t += self_attn(q, k, n)
//     t += cross_attn(norm2(t) + query_pos, memory + pos, memory);  t += ffn(norm3(t))
// from kernels that exist, in every mode: a LayerNorm launch into dnrm in front of each sub-block, the
// projections as GEMMs (the bf16 folded cross-attention query projection keeps decsa.hip's kernel), the
// attention kernels on the normed rows, and each out-projection / linear2 as a GEMM with the stream as its
// residual.  The stream alternates between tgt and dtmp (three residual adds a layer); *cur names the buffer
// that holds it.  The post-norm model's fused bf16 decoder kernels (decsa.hip) end in a LayerNorm and do not fit.
int dec_residual_gemm(Fwd& f, const Conv& c, const void* a, int lda, size_t* cur) {
  const Ws& w = f.w;
  const size_t out = *cur == w.tgt ? w.dtmp : w.tgt;
  GemmArgs g = linear_args(c, a, lda, f.Mq, f.P(out), f.d);
  g.R = f.P(*cur); g.ldr = f.d;
  CK(run_gemm(f.m, "gemm.dec", g, GEMM_LINEAR, f.s));
  *cur = out;
  return 0;
}

int decoder_layer_pre(Fwd& f, const Dec& e, int l, size_t* cur) {
  spe_model* m = f.m;
  const Ws& w = f.w;
  hipStream_t s = f.s;
  const int B = f.B, Q = f.Q, T = f.T, d = f.d, Mq = f.Mq;
  void* const n = f.P(w.dnrm);
  // ---- self-attention
  CK(run_layernorm(m, "ln.dec", f.P(*cur), e.n1g, e.n1b, n, nullptr, Mq, d, f.dt, s));
  TRY(dec_self_attention(f, e, n, nullptr, nullptr));
  TRY(dec_residual_gemm(f, e.so, f.P(w.dao), d, cur));
  // ---- cross-attention
  CK(run_layernorm(m, "ln.dec", f.P(*cur), e.n2g, e.n2b, n, nullptr, Mq, d, f.dt, s));
  if (spe_use_xattn(m)) {
    // bf16, against the memory itself: q' from n, the memory in nrm, memory + pos in srcpos
    TRY(dec_cross_query(f, e, n, nullptr));
    XattnArgs x = xattn_args(f, e, f.P(w.srcpos), d, f.P(w.nrm), d);
    const double fl = 4.0 * B * 8.0 * Q * (double)T * d + 2.0 * Mq * 8.0 * d * 32;
    const double by = 2.0 * B * (double)T * d * m->esz + 2.0 * Mq * 8.0 * d * m->esz;
    CK(run_other(m, "attn.dec_cross", fl, by, s, [&] { return spe_launch_xattn(x, s); }));
  } else {
    TRY(dec_cross_attention_projected(f, e, l, n, nullptr));
  }
  if (f.tap && f.tap->dec_map && f.tap->dec_layer == l) TRY(dec_attn_map(f, l, f.tap->dec_map));
  TRY(dec_residual_gemm(f, e.co, f.P(w.dao), d, cur));
  // ---- FFN
  CK(run_layernorm(m, "ln.dec", f.P(*cur), e.n3g, e.n3b, n, nullptr, Mq, d, f.dt, s));
  {
    GemmArgs g = linear_args(e.l1, n, d, Mq, f.P(w.dffn), f.ff);
    g.act = ACT_RELU;
    CK(run_gemm(m, "gemm.dec", g, GEMM_LINEAR, s));
  }
  return dec_residual_gemm(f, e.l2, f.P(w.dffn), f.ff, cur);
}

int decoder_stage_pre(Fwd& f, const spe_forward_outputs& out) {
  spe_model* m = f.m;
  const int L = f.L, Mq = f.Mq;
  CK((int)hipMemsetAsync(f.P(f.w.tgt), 0, (size_t)Mq * f.d * m->esz, f.s));
  size_t cur = f.w.tgt;
  for (int l = 0; l < L; ++l) {
    TRY(decoder_layer_pre(f, m->dec[l], l, &cur));
    TRY(aux_heads(f, l, f.P(cur), out));
  }
  CK(run_heads(f, f.P(cur), out.hs ? out.hs : (float*)f.P(f.w.hs), out.logits, out.points, true, out));
  return 0;
}

int forward_stages(spe_model* m, void* stream, const ImageSrc& images, int B, void* workspace, int64_t ws_bytes,
                   const spe_forward_outputs* out, int stages, const AttnTap* tap = nullptr) {
  if (!m || !workspace || B <= 0 ||
      (stages & ~(SPE_STAGE_ENCODE | SPE_STAGE_DECODE | SPE_STAGE_BACKBONE | SPE_STAGE_TRANSFORMER)) || !stages)
    return fail(SPE_E_ARG, "bad argument");
  if (stages & SPE_STAGE_ENCODE) stages |= SPE_STAGE_BACKBONE | SPE_STAGE_TRANSFORMER;
  if ((stages & SPE_STAGE_BACKBONE) && !images.f32 && !images.u8) return fail(SPE_E_ARG, "null images");
  if ((stages & SPE_STAGE_DECODE) && (!out || !out->logits || !out->points)) return fail(SPE_E_ARG, "null outputs");
  if (m->family != 0) return fail(SPE_E_ARG, "not a DETR model (use spe_rtdetr_forward)");
  if (!m->finalized) return fail(SPE_E_STATE, "model not finalized");
  const Ws w = spe_plan(m, B);
  if ((int64_t)w.total > ws_bytes) return fail(SPE_E_WORKSPACE, "workspace too small");
  const auto& c = m->cfg;
  const int F = c.input_size / spe_feat_stride(m);
  float* const amx = m->h3 ? (float*)((char*)workspace + w.amax) : nullptr;
  LedgerScope ledger(amx);
  Fwd f{m, w, (char*)workspace, (hipStream_t)stream, B, c.input_size, F, F * F, c.hidden_dim, c.dim_feedforward,
        c.num_queries, c.dec_layers, B * F * F, B * c.num_queries, c.dtype, 1.0f / std::sqrt(32.0f), amx, ledger, tap};
  // (the slot counts are checked before anything is launched: a slot handed out past its range would
  // be the encoder's input scale or a transformer slot, overwritten before an error could return)
  if (amx && (stages & SPE_STAGE_BACKBONE) && 2 + 3 * (int)m->blocks.size() + 2 > SPE_AMAX_BB - 1)
    return fail(SPE_E_STATE, "fp32h3: backbone activation-scale slots exhausted");
  if (amx && (stages & SPE_STAGE_TRANSFORMER) && 2 * (int)m->enc.size() > SPE_AMAX_DEC - SPE_AMAX_BB - 1)
    return fail(SPE_E_STATE, "fp32h3: encoder activation-scale slots exhausted");
  if (amx && (stages & SPE_STAGE_DECODE) && 3 * c.dec_layers > SPE_AMAX_SLOTS - SPE_AMAX_DEC)
    return fail(SPE_E_STATE, "fp32h3: decoder activation-scale slots exhausted");
  if (stages & SPE_STAGE_BACKBONE) TRY(backbone_stage(f, images));
  if (stages & SPE_STAGE_TRANSFORMER) TRY(m->pre_norm ? encoder_stage_pre(f) : encoder_stage(f));
  if (stages & SPE_STAGE_DECODE) TRY(m->pre_norm ? decoder_stage_pre(f, *out) : decoder_stage(f, *out));
  return 0;
}

}  // namespace

extern "C" {

int spe_forward(spe_model* m, void* stream, const float* images, int B, void* workspace, int64_t ws_bytes,
                const spe_forward_outputs* out) {
  return spe_forward_stages(m, stream, images, B, workspace, ws_bytes, out, SPE_STAGE_ENCODE | SPE_STAGE_DECODE);
}

int spe_forward_stages(spe_model* m, void* stream, const float* images, int B, void* workspace, int64_t ws_bytes,
                       const spe_forward_outputs* out, int stages) {
  return forward_stages(m, stream, ImageSrc{images, nullptr, 0}, B, workspace, ws_bytes, out, stages);
}

int spe_forward_stages_u8(spe_model* m, void* stream, const uint8_t* crops, int channels, int B, void* workspace,
                          int64_t ws_bytes, const spe_forward_outputs* out, int stages) {
  if ((stages & (SPE_STAGE_ENCODE | SPE_STAGE_BACKBONE)) && (!crops || (channels != 1 && channels != 3)))
    return fail(SPE_E_ARG, "u8 crops: device pointer, 1 or 3 channels");
  return forward_stages(m, stream, ImageSrc{nullptr, crops, channels}, B, workspace, ws_bytes, out, stages);
}

int64_t spe_forward_attention_workspace_bytes(const spe_model* m, int B) {
  // (every mode the taps serve reads operands the forward pass leaves in its own workspace)
  return spe_model_workspace_bytes(m, B);
}

int spe_forward_attention(spe_model* m, void* stream, const float* images, int B, void* workspace, int64_t ws_bytes,
                          const spe_forward_outputs* out, int enc_layer, int dec_layer, float* enc_map,
                          float* dec_map) {
  if (!m) return fail(SPE_E_ARG, "bad argument");
  if (m->family != 0) return fail(SPE_E_ARG, "not a DETR model (attention maps: the DETR keypoint model only)");
  if (m->x3)
    return fail(SPE_E_ARG, "attention maps: supported modes are bf16 (attn_dtype fp16 included) and fp32; the "
                           "split-precision modes (fp32x3 / fp32x6 / fp32h3) keep their operands as split planes");
  if (!enc_map && !dec_map) return fail(SPE_E_ARG, "attention maps: enc_map and dec_map are both null");
  const int EL = m->cfg.enc_layers, DL = m->cfg.dec_layers;
  AttnTap tap{enc_layer < 0 ? enc_layer + EL : enc_layer, dec_layer < 0 ? dec_layer + DL : dec_layer, enc_map, dec_map};
  if (enc_map && (tap.enc_layer < 0 || tap.enc_layer >= EL)) return fail(SPE_E_ARG, "attention maps: enc_layer out of range");
  if (dec_map && (tap.dec_layer < 0 || tap.dec_layer >= DL)) return fail(SPE_E_ARG, "attention maps: dec_layer out of range");
  return forward_stages(m, stream, ImageSrc{images, nullptr, 0}, B, workspace, ws_bytes, out,
                        SPE_STAGE_ENCODE | SPE_STAGE_DECODE, &tap);
}

}  // extern "C"
