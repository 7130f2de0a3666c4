// MobileNetV3_Large / MobileNetV3_Small backbones of the RT-DETR runtime (UNC/nn/backbone/mobilenetv3.py:123-320):
// parameter keys, packing and the launch sequence behind the RtBackbone row rt_bb_mbv3; mb_table() is the one
// place that tells the two variants apart.  Also the packing and launch helpers GhostNetV2 shares
// (rtdetr_backbone.h).
#include <cmath>

#include "rtdetr_backbone.h"

#define fail spe_fail

// ---- shared with GhostNetV2 (the BatchNorm fold is registry.cpp's bn_fold; MobileNetV3_Small's bare Conv1 / Conv2: "")
// conv [cout][cin][kh][kw] (+ a bias in front of the norm) + BatchNorm -> rows [cout][(y*kw + x)*cin + ci]
// (the plain tap-major K order mb_gemm's A loader walks), folded bias.  pool2: the conv reads a 2x2 mean
// of its input -- folded into a (2kh)x(2kw) kernel of stride 2*stride, pad 2*pad, w/4 per tap (exact).
Conv mb_conv(spe_model* m, const std::string& wkey, const std::string& bn, const std::string& biaskey, int stride,
             int pad, bool pool2) {
  const auto sh = param_shape(m, wkey);
  const int cout = (int)sh[0], cin = (int)sh[1], kh = (int)sh[2], kw = (int)sh[3];
  const int f = pool2 ? 2 : 1, KH = kh * f, KW = kw * f, K = KH * KW * cin;
  std::vector<double> scale, shift;
  bn_fold(m, bn, cout, scale, shift);
  const auto& w = m->host[wkey];
  std::vector<float> rows((size_t)cout * K, 0.f), bias(cout);
  for (int co = 0; co < cout; ++co) {
    if (!biaskey.empty()) shift[co] += (double)m->host[biaskey][co] * scale[co];
    bias[co] = (float)shift[co];
    for (int ci = 0; ci < cin; ++ci)
      for (int y = 0; y < KH; ++y)
        for (int x = 0; x < KW; ++x)
          rows[(size_t)co * K + (size_t)(y * KW + x) * cin + ci] =
              (float)((double)w[(((size_t)co * cin + ci) * kh + y / f) * kw + x / f] * scale[co] / (f * f));
  }
  Conv c = rows_conv(m, rows, cout, K, bias.data(), bias.size());
  c.Cin = cin; c.KH = KH; c.KW = KW; c.stride = stride * f; c.pad = pad * f;
  return c;
}

MbDw mb_dw(spe_model* m, const std::string& wkey, const std::string& bn, int stride) {
  const auto sh = param_shape(m, wkey);
  const int C = (int)sh[0], k = (int)sh[2];
  std::vector<double> scale, shift;
  bn_fold(m, bn, C, scale, shift);
  const auto& w = m->host[wkey];
  std::vector<float> wt((size_t)k * k * C), bias(C);
  for (int c = 0; c < C; ++c) {
    bias[c] = (float)shift[c];
    for (int t = 0; t < k * k; ++t) wt[(size_t)t * C + c] = (float)((double)w[(size_t)c * k * k + t] * scale[c]);
  }
  MbDw d;
  d.C = C; d.k = k; d.stride = stride;
  d.w = upload_f32(m, wt.data(), wt.size());
  d.bias = upload_f32(m, bias.data(), bias.size());
  return d;
}

int mb_run_pw(const MbRun& x, const Conv& cv, const void* in, int Hin, void* outp, int act, const void* R, const float* scale) {
  MbGemmArgs g{};
  const int B = x.B, Ho = (Hin + 2 * cv.pad - cv.KH) / cv.stride + 1;
  g.A = in; g.lda = cv.Cin;
  g.Bw = cv.w; g.ldb = cv.Kpad;
  g.bias = cv.bias; g.scale = scale;
  g.R = R; g.ldr = cv.N;
  g.C = outp; g.ldc = cv.N;
  g.M = B * Ho * Ho; g.N = cv.N; g.K = cv.K;
  g.H = Hin; g.W = Hin; g.Cin = cv.Cin; g.KH = cv.KH; g.KW = cv.KW; g.stride = cv.stride; g.pad = cv.pad;
  g.Ho = Ho; g.Wo = Ho;
  g.act = act;
  const double a_elems = (double)B * Hin * Hin * cv.Cin, E = x.m->esz;
  return run_other(x.m, "conv.pw.mb", 2.0 * g.M * g.N * g.K,
                   (a_elems + (double)g.N * g.K + (double)g.M * g.N * (R ? 2 : 1)) * E, x.s,
                   [&] { return spe_launch_mb_gemm(g, x.m->rt->cfg.dtype, x.s); });
}

int mb_run_dw(const MbRun& x, const MbDw& d, const void* in, int Hin, void* outp, int act, float* pool) {
  MbDwArgs a{};
  const int B = x.B;
  a.in = in; a.out = outp; a.w = d.w; a.bias = d.bias; a.pool = pool;
  a.B = B; a.H = Hin; a.W = Hin; a.C = d.C; a.k = d.k; a.stride = d.stride; a.act = act;
  const int Ho = Hin / d.stride;
  const double E = x.m->esz;
  return run_other(x.m, "conv.dw", 2.0 * B * Ho * Ho * d.C * d.k * d.k, (double)B * d.C * (Hin * Hin + Ho * Ho) * E, x.s,
                   [&] { return spe_launch_mb_dwconv(a, x.m->rt->cfg.dtype, x.s); });
}

int mb_run_se(const MbRun& x, const MbSe& g, const float* pool, int tiles, int Ho, int C, float* scale) {
  MbSeArgs a{};
  const int B = x.B;
  a.pool = pool; a.tiles = tiles; a.inv_hw = 1.0f / (float)(Ho * Ho);
  a.w1 = g.w1; a.b1 = g.b1; a.w2t = g.w2t; a.b2 = g.b2;
  a.scale = scale;
  a.B = B; a.C = C; a.hidden = g.hidden;
  return run_other(x.m, "rt.se", 4.0 * B * C * g.hidden, ((double)B * (tiles + 1) * C + 2.0 * C * g.hidden) * 4, x.s,
                   [&] { return spe_launch_mb_se_gate(a, x.s); });
}

namespace {

// MobileNetV3_Large.bneck (mobilenetv3.py:148-164): kernel, in, expand, out, Hardswish (else ReLU), SE, stride
struct MbRow { int k, cin, cexp, cout, hs, se, stride; };
const MbRow MBV3_LARGE[15] = {
    {3, 16, 16, 16, 0, 0, 1},    {3, 16, 64, 24, 0, 0, 2},    {3, 24, 72, 24, 0, 0, 1},   {5, 24, 72, 40, 0, 1, 2},
    {5, 40, 120, 40, 0, 1, 1},   {5, 40, 120, 40, 0, 1, 1},   {3, 40, 240, 80, 1, 0, 2},  {3, 80, 200, 80, 1, 0, 1},
    {3, 80, 184, 80, 1, 0, 1},   {3, 80, 184, 80, 1, 0, 1},   {3, 80, 480, 112, 1, 1, 1}, {3, 112, 672, 112, 1, 1, 1},
    {5, 112, 672, 160, 1, 1, 2}, {5, 160, 672, 160, 1, 1, 1}, {5, 160, 960, 160, 1, 1, 1}};
// MobileNetV3_Small.bneck (mobilenetv3.py:248-260).  Block 0: full stem resolution, SE, stride 2 with in == out
const MbRow MBV3_SMALL[11] = {
    {3, 16, 16, 16, 0, 1, 2},  {3, 16, 72, 24, 0, 0, 2},  {3, 24, 88, 24, 0, 0, 1},  {5, 24, 96, 40, 1, 1, 2},
    {5, 40, 240, 40, 1, 1, 1}, {5, 40, 240, 40, 1, 1, 1}, {5, 40, 120, 48, 1, 1, 1}, {5, 48, 144, 48, 1, 1, 1},
    {5, 48, 288, 96, 1, 1, 2}, {5, 96, 576, 96, 1, 1, 1}, {5, 96, 576, 96, 1, 1, 1}};
struct MbTable { const MbRow* rows; int n, last_in, head_in; bool small; };   // conv2's and linear3's input widths
inline MbTable mb_table(const spe_rtdetr_config& c) {
  return c.depth == SPE_RTDETR_MBV3_SMALL ? MbTable{MBV3_SMALL, 11, 96, 576, true} : MbTable{MBV3_LARGE, 15, 160, 960, false};
}
inline int se_hidden(int c) { return c / 4 > 8 ? c / 4 : 8; }

// registration order of MobileNetV3_{Large,Small}.__init__ (mobilenetv3.py:136-173, 241-270)
void mbv3_spec(const spe_rtdetr_config& c, RtSpec& s) {
  const std::string b = "backbone.";
  const MbTable t = mb_table(c);
  s.add(b + "conv1.weight", {16, 3, 3, 3});
  if (!t.small) { s.bn(b + "bn1", 16); s.bn(b + "Bn1", 128); s.bn(b + "Bn2", 256); }
  s.add(b + "Conv1.weight", {128, 16, 3, 3});
  s.add(b + "Conv2.weight", {256, 128, 3, 3});
  if (t.small) s.bn(b + "bn1", 16);       // Small: Conv1 / Conv2 are bare, bn1 is registered after them
  for (int i = 0; i < t.n; ++i) {
    const MbRow& r = t.rows[i];
    const std::string p = b + "bneck." + std::to_string(i);
    s.add(p + ".conv1.weight", {r.cexp, r.cin, 1, 1}); s.bn(p + ".bn1", r.cexp);
    s.add(p + ".conv2.weight", {r.cexp, 1, r.k, r.k}); s.bn(p + ".bn2", r.cexp);
    if (r.se) {
      const int64_t h = se_hidden(r.cexp);
      s.add(p + ".se.se.1.weight", {h, r.cexp, 1, 1}); s.bn(p + ".se.se.2", h);
      s.add(p + ".se.se.4.weight", {r.cexp, h, 1, 1});
    }
    s.add(p + ".conv3.weight", {r.cout, r.cexp, 1, 1}); s.bn(p + ".bn3", r.cout);
    if (r.stride == 1 && r.cin != r.cout) {
      s.add(p + ".skip.0.weight", {r.cout, r.cin, 1, 1}); s.bn(p + ".skip.1", r.cout);
    } else if (r.stride == 2 && r.cin != r.cout) {
      s.add(p + ".skip.0.weight", {r.cin, 1, 3, 3}); s.bn(p + ".skip.1", r.cin);
      s.add(p + ".skip.2.weight", {r.cout, r.cin, 1, 1}); s.add(p + ".skip.2.bias", {r.cout}); s.bn(p + ".skip.3", r.cout);
    } else if (r.stride == 2) {
      s.add(p + ".skip.0.weight", {r.cout, 1, 3, 3}); s.bn(p + ".skip.1", r.cout);
    }
  }
  s.add(b + "conv2.weight", {512, t.last_in, 1, 1}); s.bn(b + "bn2", 512);
  s.add(b + "linear3.weight", {1280, t.head_in}); s.bn(b + "bn3", 1280);     // built, never called
}

int build_mbv3(spe_model* m) {
  RtMbv3& mb = m->rt->mb;
  const std::string b = "backbone.";
  const MbTable tab = mb_table(m->rt->cfg);
  const bool small = tab.small;
  std::vector<float> entry(MBS_W_FLOATS, 0.f);     // Small: mbs_entry's weights (spe_kernels.h, MBS_W_*)
  {   // conv1 + bn1: fp32 [27][16] with k = (ci*3 + kh)*3 + kw
    std::vector<double> scale, shift;
    bn_fold(m, b + "bn1", 16, scale, shift);
    const auto& w = m->host[b + "conv1.weight"];
    std::vector<float> wt(27 * 16), bias(16);
    for (int c = 0; c < 16; ++c) {
      bias[c] = (float)shift[c];
      for (int k = 0; k < 27; ++k) wt[(size_t)k * 16 + c] = (float)((double)w[(size_t)c * 27 + k] * scale[c]);
    }
    mb.stem_w = upload_f32(m, wt.data(), wt.size());
    mb.stem_b = upload_f32(m, bias.data(), bias.size());
    std::copy(wt.begin(), wt.end(), entry.begin() + MBS_W_STEM);
    std::copy(bias.begin(), bias.end(), entry.begin() + MBS_W_STEM_B);
  }
  // Small: Conv1 / Conv2 are bare convolutions (no BatchNorm, no activation)
  mb.side_act = small ? MB_ACT_NONE : MB_ACT_HSWISH;
  mb.conv_b = mb_conv(m, b + "Conv1.weight", small ? "" : b + "Bn1", "", 2, 1, true);
  if (small) mb.conv_b3 = mb_conv(m, b + "Conv1.weight", "", "", 2, 1);     // over mbs_entry's pooled map
  mb.conv_c = mb_conv(m, b + "Conv2.weight", small ? "" : b + "Bn2", "", 2, 1);
  mb.blocks.clear();
  for (int i = 0; i < tab.n; ++i) {
    const MbRow& r = tab.rows[i];
    const std::string p = b + "bneck." + std::to_string(i);
    MbBlock k;
    k.cin = r.cin; k.cexp = r.cexp; k.cout = r.cout; k.stride = r.stride;
    k.act = r.hs ? MB_ACT_HSWISH : MB_ACT_RELU;
    k.expand = mb_conv(m, p + ".conv1.weight", p + ".bn1", "", 1, 0);
    k.dw = mb_dw(m, p + ".conv2.weight", p + ".bn2", r.stride);
    k.se = r.se != 0;
    if (k.se) {
      const int h = se_hidden(r.cexp), C = r.cexp;
      k.gate.hidden = h;
      std::vector<double> scale, shift;
      bn_fold(m, p + ".se.se.2", h, scale, shift);
      const auto& w1 = m->host[p + ".se.se.1.weight"];
      const auto& w2 = m->host[p + ".se.se.4.weight"];
      std::vector<float> f1((size_t)h * C), b1(h), f2t((size_t)h * C);
      for (int j = 0; j < h; ++j) {
        b1[j] = (float)shift[j];
        for (int c = 0; c < C; ++c) {
          f1[(size_t)j * C + c] = (float)((double)w1[(size_t)j * C + c] * scale[j]);
          f2t[(size_t)j * C + c] = w2[(size_t)c * h + j];
        }
      }
      k.gate.w1 = upload_f32(m, f1.data(), f1.size());
      k.gate.b1 = upload_f32(m, b1.data(), b1.size());
      k.gate.w2t = upload_f32(m, f2t.data(), f2t.size());
    }
    k.project = mb_conv(m, p + ".conv3.weight", p + ".bn3", "", 1, 0);
    if (r.stride == 1 && r.cin != r.cout) {
      k.has_skip_pw = true;
      k.skip_pw = mb_conv(m, p + ".skip.0.weight", p + ".skip.1", "", 1, 0);
    } else if (r.stride == 2) {
      k.has_skip_dw = true;
      k.skip_dw = mb_dw(m, p + ".skip.0.weight", p + ".skip.1", 2);
      if (r.cin != r.cout) {
        k.has_skip_pw = true;
        k.skip_pw = mb_conv(m, p + ".skip.2.weight", p + ".skip.3", p + ".skip.2.bias", 1, 0);
      }
    }
    mb.blocks.push_back(k);
  }
  mb.last = mb_conv(m, b + "conv2.weight", b + "bn2", "", 1, 0);
  if (small) {     // block 0's expand [ci][co], depthwise and skip depthwise [9][16], fp32 with BatchNorm folded
    const std::string p = b + "bneck.0";
    std::vector<double> scale, shift;
    bn_fold(m, p + ".bn1", 16, scale, shift);
    const auto& w1 = m->host[p + ".conv1.weight"];
    for (int co = 0; co < 16; ++co) {
      entry[MBS_W_EXP_B + co] = (float)shift[co];
      for (int ci = 0; ci < 16; ++ci) entry[MBS_W_EXP + ci * 16 + co] = (float)((double)w1[(size_t)co * 16 + ci] * scale[co]);
    }
    const char* dwk[2][2] = {{".conv2.weight", ".bn2"}, {".skip.0.weight", ".skip.1"}};
    const int off[2][2] = {{MBS_W_DW, MBS_W_DW_B}, {MBS_W_SKIP, MBS_W_SKIP_B}};
    for (int j = 0; j < 2; ++j) {
      bn_fold(m, p + dwk[j][1], 16, scale, shift);
      const auto& w = m->host[p + dwk[j][0]];
      for (int c = 0; c < 16; ++c) {
        entry[off[j][1] + c] = (float)shift[c];
        for (int t = 0; t < 9; ++t) entry[off[j][0] + t * 16 + c] = (float)((double)w[(size_t)c * 9 + t] * scale[c]);
      }
    }
    mb.entry_w = upload_f32(m, entry.data(), entry.size());
  }
  return 0;
}

// MobileNetV3_Large.forward / MobileNetV3_Small.forward (mobilenetv3.py:206-225, 301-320) at input 256: stem ->
// x0 [B][128][128][16]; Conv1 (2x2 mean folded in) -> f0, Conv2 -> f1; the 15 blocks ping-pong bufA / bufB with the expanded tensor in t1,
// the depthwise output in t2 and the skip branch in sc; conv2 -> f2.  Small with the fused entry (mbs_entry,
// SPE_MBS_ENTRY, default on): one launch leaves the 2x2 mean of the stem map in x0 [B][64][64][16] (Conv1 reads
// it as a plain 3x3/s2), block 0's skip in sc and its depthwise output in t2 with the SE pool partials; the
// block loop then starts at block 0's SE gate.
int rt_backbone_mbv3(spe_model* m, hipStream_t s, const ImageSrc& images, int B, char* ws, const RtWs& w) {
  const RtModel& r = *m->rt;
  const RtMbv3& mb = r.mb;
  const int dt = r.cfg.dtype, S = r.cfg.input_size;
  const double E = m->esz;
  auto P = [&](size_t o) { return (void*)(ws + o); };
  const MbRun x{m, s, B};
  const int H0 = S / 2;
  const bool fused = mb_table(r.cfg).small && spe_mbs_entry_enabled();
  if (fused) {
    if ((size_t)spe_mbs_entry_tiles(S) * 16 > MB_POOL_MAX) return fail(SPE_E_WORKSPACE, "SE pool partials exceed the plan");
    MbsEntryArgs a{};
    a.src = images; a.w = mb.entry_w;
    a.pooled = P(w.x0); a.skip = P(w.sc); a.t2 = P(w.t2); a.pool = (float*)P(w.mbpool);
    a.B = B; a.S = S;
    const double px = (double)B * (S / 4) * (S / 4);
    CK(run_other(m, "conv.entry.mbs", 2.0 * px * 16 * (4 * 27 + 4 * 16 + 9 + 9),
                 (double)B * S * S * image_px_bytes(images) + 3.0 * px * 16 * E, s,
                 [&] { return spe_launch_mbs_entry(a, dt, s); }));
    CK(mb_run_pw(x, mb.conv_b3, P(w.x0), S / 4, P(w.f0), mb.side_act, nullptr, nullptr));
  } else {
    CK(run_other(m, "conv.stem.mb", 2.0 * B * H0 * H0 * 16 * 27,
                 (double)B * (S * S * image_px_bytes(images) + H0 * H0 * 16 * E), s,
                 [&] { return spe_launch_mb_stem(images, mb.stem_w, mb.stem_b, P(w.x0), B, S, dt, s); }));
    CK(mb_run_pw(x, mb.conv_b, P(w.x0), H0, P(w.f0), mb.side_act, nullptr, nullptr));
  }
  CK(mb_run_pw(x, mb.conv_c, P(w.f0), r.lvl_s[0], P(w.f1), mb.side_act, nullptr, nullptr));
  int H = H0;
  size_t cur = w.x0;
  const size_t sc_pw = w.sc + (((w.f0 - w.sc) / 2) & ~size_t(255));   // second half of sc: the skip branch's 1x1 output
  bool entry_done = fused;             // block 0's expand, depthwise and skip are already in t2 / sc
  for (const MbBlock& k : mb.blocks) {
    const int Ho = H / k.stride;
    const size_t outbuf = cur == w.bufA ? w.bufB : w.bufA;
    const bool head = entry_done;
    entry_done = false;
    if (!head) CK(mb_run_pw(x, k.expand, P(cur), H, P(w.t1), k.act, nullptr, nullptr));
    float* pool = nullptr;
    const int tiles = spe_mb_dwconv_tiles(Ho, Ho);
    if (k.se) {
      if ((size_t)tiles * k.cexp > MB_POOL_MAX) return fail(SPE_E_WORKSPACE, "SE pool partials exceed the plan");
      pool = (float*)P(w.mbpool);      // rows [B][tiles][C]: B * tiles * C <= B * MB_POOL_MAX floats
    }
    if (!head) CK(mb_run_dw(x, k.dw, P(w.t1), H, P(w.t2), k.act, pool));
    const float* scale = nullptr;
    if (k.se) {
      CK(mb_run_se(x, k.gate, pool, tiles, Ho, k.cexp, (float*)P(w.mbscale)));
      scale = (const float*)P(w.mbscale);
    }
    const void* res = P(cur);
    if (k.has_skip_dw) {
      if (!head) CK(mb_run_dw(x, k.skip_dw, P(cur), H, P(w.sc), MB_ACT_NONE, nullptr));
      res = P(w.sc);
    }
    if (k.has_skip_pw) {
      CK(mb_run_pw(x, k.skip_pw, res, k.has_skip_dw ? Ho : H, P(sc_pw), MB_ACT_NONE, nullptr, nullptr));
      res = P(sc_pw);
    }
    CK(mb_run_pw(x, k.project, P(w.t2), Ho, P(outbuf), k.act, res, scale));
    H = Ho;
    cur = outbuf;
  }
  CK(mb_run_pw(x, mb.last, P(cur), H, P(w.f2), MB_ACT_HSWISH, nullptr, nullptr));
  return 0;
}

const char* mbv3_refuses(const spe_rtdetr_config& c) {
  return c.input_size == 256 ? nullptr
                             : "MobileNetV3_Large / _Small support input_size 256 only: the backbone resizes its stem output to "
                               "a hard-coded 64x64, which is the stride-4 grid the stride-8 / 16 levels are built from "
                               "only at 256";
}

}  // namespace

const RtBackbone* rt_bb_mbv3() {
  static const RtBackbone bb = {
      [](const spe_rtdetr_config& c) { return c.depth == SPE_RTDETR_MBV3_LARGE || c.depth == SPE_RTDETR_MBV3_SMALL; },
      mbv3_refuses,
      [](const spe_rtdetr_config&, int fch[3]) { fch[0] = 128; fch[1] = 256; fch[2] = 512; },
      mbv3_spec, build_mbv3, rt_backbone_mbv3, true};
  return &bb;
}

