// GhostNetV2 backbone of the RT-DETR runtime (UNC/nn/backbone/ghostnetv2.py:88-441): parameter keys, packing in the
// padded ghost layout and the launch sequence behind the RtBackbone row rt_bb_ghostv2.  The 1x1 / implicit-GEMM
// convs, the depthwise convs and the SE gate go through the launch helpers shared with MobileNetV3
// (rtdetr_backbone.h).
#include "rtdetr_backbone.h"

#define fail spe_fail

namespace {

// GhostNetV2.cfgs at width 1.0 (ghostnetv2.py:297-319) in layer_id order: dw kernel, mid, out, SE, stride, and
// the nn.Sequential stage / index the block's key carries.  Blocks 0-1: ghost1 mode "original", >= 2: "attn".
struct GhRow { int k, mid, cout, se, stride, stage, idx; };
const GhRow GHOSTV2[16] = {
    {3, 16, 16, 0, 1, 0, 0},   {3, 48, 24, 0, 2, 1, 0},   {3, 72, 24, 0, 1, 2, 0},   {5, 72, 40, 1, 2, 3, 0},
    {5, 120, 40, 1, 1, 4, 0},  {3, 240, 80, 0, 2, 5, 0},  {3, 200, 80, 0, 1, 6, 0},  {3, 184, 80, 0, 1, 6, 1},
    {3, 184, 80, 0, 1, 6, 2},  {3, 480, 112, 1, 1, 6, 3}, {3, 672, 112, 1, 1, 6, 4}, {5, 672, 160, 1, 2, 7, 0},
    {5, 960, 160, 0, 1, 8, 0}, {5, 960, 160, 1, 1, 8, 1}, {5, 960, 160, 0, 1, 8, 2}, {5, 960, 160, 1, 1, 8, 3}};
constexpr int GH_ATTN_FROM = 2;
// SqueezeExcite's reduced width, _make_divisible(mid * 0.25, 4) (ghostnetv2.py:21-34): 20, 32, 120, 168, 240
inline int gh_se_hidden(int mid) {
  const double v = mid * 0.25;
  int n = (int)(v + 2) / 4 * 4;
  if (n < 4) n = 4;
  return n < 0.9 * v ? n + 4 : n;
}
inline std::string gh_key(const GhRow& r) { return "backbone.blocks." + std::to_string(r.stage) + "." + std::to_string(r.idx); }
// physical layout of a C-channel ghost tensor: two halves of hp = pad8(C / 2) lanes (identity when C / 2 % 8 == 0)
struct GhLay {
  int C, half, hp;
  explicit GhLay(int c) : C(c), half(c / 2), hp((c / 2 + 7) & ~7) {}
  int Cp() const { return 2 * hp; }
  int phys(int c) const { return c < half ? c : hp + c - half; }
};

// registration order of GhostNetV2.__init__ (ghostnetv2.py:331-387)
void ghost_spec(const spe_rtdetr_config&, RtSpec& s) {
  const std::string b = "backbone.";
  s.bn(b + "Bn1", 128); s.bn(b + "Bn2", 256); s.bn(b + "Bn3", 512);
  s.add(b + "Conv1.weight", {128, 16, 3, 3});
  s.add(b + "Conv2.weight", {256, 128, 3, 3});
  s.add(b + "Conv3.weight", {512, 960, 1, 1});
  s.add(b + "conv_stem.weight", {16, 3, 3, 3});
  s.bn(b + "bn1", 16);
  auto ghost = [&](const std::string& p, int64_t cin, int64_t cout, bool attn) {
    const int64_t h = (cout + 1) / 2;
    s.add(p + ".primary_conv.0.weight", {h, cin, 1, 1}); s.bn(p + ".primary_conv.1", h);
    s.add(p + ".cheap_operation.0.weight", {h, 1, 3, 3}); s.bn(p + ".cheap_operation.1", h);
    if (attn) {
      s.add(p + ".short_conv.0.weight", {cout, cin, 1, 1}); s.bn(p + ".short_conv.1", cout);
      s.add(p + ".short_conv.2.weight", {cout, 1, 1, 5}); s.bn(p + ".short_conv.3", cout);
      s.add(p + ".short_conv.4.weight", {cout, 1, 5, 1}); s.bn(p + ".short_conv.5", cout);
    }
  };
  int64_t cin = 16;
  for (int i = 0; i < 16; ++i) {
    const GhRow& r = GHOSTV2[i];
    const std::string p = gh_key(r);
    ghost(p + ".ghost1", cin, r.mid, i >= GH_ATTN_FROM);
    if (r.stride > 1) { s.add(p + ".conv_dw.weight", {r.mid, 1, r.k, r.k}); s.bn(p + ".bn_dw", r.mid); }
    if (r.se) {
      const int64_t h = gh_se_hidden(r.mid);
      s.add(p + ".se.conv_reduce.weight", {h, r.mid, 1, 1}); s.add(p + ".se.conv_reduce.bias", {h});
      s.add(p + ".se.conv_expand.weight", {r.mid, h, 1, 1}); s.add(p + ".se.conv_expand.bias", {r.mid});
    }
    ghost(p + ".ghost2", r.mid, r.cout, false);
    if (!(cin == r.cout && r.stride == 1)) {
      s.add(p + ".shortcut.0.weight", {cin, 1, r.k, r.k}); s.bn(p + ".shortcut.1", cin);
      s.add(p + ".shortcut.2.weight", {r.cout, cin, 1, 1}); s.bn(p + ".shortcut.3", r.cout);
    }
    cin = r.cout;
  }
  s.add(b + "blocks.9.0.conv.weight", {960, 160, 1, 1}); s.bn(b + "blocks.9.0.bn1", 960);
  s.add(b + "conv_head.weight", {1280, 960, 1, 1}); s.add(b + "conv_head.bias", {1280});   // built, never called
  s.lin(b + "classifier", 1000, 1280);
}

// ---- GhostNetV2 packing.  Inputs and outputs of every conv are in the padded ghost layout (GhLay): weights
// of a pad lane, as an input column or an output row, and its bias are zero.
// 1x1 conv [cout][cin] + BatchNorm -> rows [N][Cp(cin)]; half_out: the output is a ghost half (N = pad8(cout),
// rows in order), else a whole ghost tensor (N = Cp(cout), rows at GhLay(cout).phys)
Conv gh_pw(spe_model* m, const std::string& conv, const std::string& bn, bool half_out) {
  const auto sh = param_shape(m, conv + ".weight");
  const int cout = (int)sh[0], cin = (int)sh[1];
  const GhLay li(cin), lo(cout);
  const int K = li.Cp(), N = half_out ? (cout + 7) & ~7 : lo.Cp();
  std::vector<double> scale, shift;
  bn_fold(m, bn, cout, scale, shift);
  const auto& w = m->host[conv + ".weight"];
  std::vector<float> rows((size_t)N * K, 0.f), bias(N, 0.f);
  for (int co = 0; co < cout; ++co) {
    const int n = half_out ? co : lo.phys(co);
    bias[n] = (float)shift[co];
    for (int ci = 0; ci < cin; ++ci) rows[(size_t)n * K + li.phys(ci)] = (float)((double)w[(size_t)co * cin + ci] * scale[co]);
  }
  return rows_conv(m, rows, N, K, bias.data(), bias.size());
}

// depthwise conv [C][1][kh][kw] + BatchNorm -> fp32 taps [kh*kw][Cp] and bias [Cp]; half: C is a ghost half
// (lanes in order, Cp = pad8(C)), else a whole ghost tensor
void gh_dw_pack(spe_model* m, const std::string& conv, const std::string& bn, bool half, float** wd, float** bd, int* Cp,
                int* k) {
  const auto sh = param_shape(m, conv + ".weight");
  const int C = (int)sh[0], taps = (int)(sh[2] * sh[3]);
  const GhLay l(C);
  const int P = half ? (C + 7) & ~7 : l.Cp();
  std::vector<double> scale, shift;
  bn_fold(m, bn, C, scale, shift);
  const auto& w = m->host[conv + ".weight"];
  std::vector<float> wt((size_t)taps * P, 0.f), bias(P, 0.f);
  for (int c = 0; c < C; ++c) {
    const int pc = half ? c : l.phys(c);
    bias[pc] = (float)shift[c];
    for (int t = 0; t < taps; ++t) wt[(size_t)t * P + pc] = (float)((double)w[(size_t)c * taps + t] * scale[c]);
  }
  *wd = upload_f32(m, wt.data(), wt.size());
  *bd = upload_f32(m, bias.data(), bias.size());
  if (Cp) *Cp = P;
  if (k) *k = (int)sh[2];
}

MbDw gh_dw(spe_model* m, const std::string& conv, const std::string& bn, int stride) {
  MbDw d;
  gh_dw_pack(m, conv, bn, false, &d.w, &d.bias, &d.C, &d.k);
  d.stride = stride;
  return d;
}

GhModule gh_module(spe_model* m, const std::string& p, bool attn) {
  GhModule g;
  g.primary = gh_pw(m, p + ".primary_conv.0", p + ".primary_conv.1", true);
  gh_dw_pack(m, p + ".cheap_operation.0", p + ".cheap_operation.1", true, &g.cheap_w, &g.cheap_b, &g.half_p, nullptr);
  g.attn = attn;
  if (attn) {
    g.short_pw = gh_pw(m, p + ".short_conv.0", p + ".short_conv.1", false);
    gh_dw_pack(m, p + ".short_conv.2", p + ".short_conv.3", false, &g.dfc_w1, &g.dfc_b1, nullptr, nullptr);
    gh_dw_pack(m, p + ".short_conv.4", p + ".short_conv.5", false, &g.dfc_w2, &g.dfc_b2, nullptr, nullptr);
  }
  return g;
}

int build_ghost(spe_model* m) {
  RtGhost& gh = m->rt->gh;
  const std::string b = "backbone.";
  {   // conv_stem: fp32 [27][16] with k = (ci*3 + kh)*3 + kw; bn1 stays apart (the raw output is needed too)
    std::vector<double> scale, shift;
    bn_fold(m, b + "bn1", 16, scale, shift);
    const auto& w = m->host[b + "conv_stem.weight"];
    std::vector<float> wt(27 * 16), sc(16), sf(16);
    for (int c = 0; c < 16; ++c) {
      sc[c] = (float)scale[c];
      sf[c] = (float)shift[c];
      for (int k = 0; k < 27; ++k) wt[(size_t)k * 16 + c] = w[(size_t)c * 27 + k];
    }
    gh.stem_w = upload_f32(m, wt.data(), wt.size());
    gh.stem_scale = upload_f32(m, sc.data(), sc.size());
    gh.stem_shift = upload_f32(m, sf.data(), sf.size());
  }
  gh.conv_b = mb_conv(m, b + "Conv1.weight", b + "Bn1", "", 2, 1, true);
  gh.conv_c = mb_conv(m, b + "Conv2.weight", b + "Bn2", "", 2, 1);
  gh.blocks.clear();
  int cin = 16;
  for (int i = 0; i < 16; ++i) {
    const GhRow& r = GHOSTV2[i];
    const std::string p = gh_key(r);
    GhBlock k;
    k.cin_p = GhLay(cin).Cp(); k.mid_p = GhLay(r.mid).Cp(); k.cout_p = GhLay(r.cout).Cp();
    k.k = r.k; k.stride = r.stride;
    k.g1 = gh_module(m, p + ".ghost1", i >= GH_ATTN_FROM);
    if (r.stride > 1) k.dw = gh_dw(m, p + ".conv_dw", p + ".bn_dw", r.stride);
    k.se = r.se != 0;
    if (k.se) {
      const int h = gh_se_hidden(r.mid), C = r.mid, Cp = k.mid_p;
      const GhLay l(C);
      k.gate.hidden = h;
      const auto& w1 = m->host[p + ".se.conv_reduce.weight"];
      const auto& w2 = m->host[p + ".se.conv_expand.weight"];
      const auto& b2 = m->host[p + ".se.conv_expand.bias"];
      std::vector<float> f1((size_t)h * Cp, 0.f), f2t((size_t)h * Cp, 0.f), fb2(Cp, 0.f);
      for (int c = 0; c < C; ++c) {
        fb2[l.phys(c)] = b2[c];
        for (int j = 0; j < h; ++j) {
          f1[(size_t)j * Cp + l.phys(c)] = w1[(size_t)j * C + c];
          f2t[(size_t)j * Cp + l.phys(c)] = w2[(size_t)c * h + j];
        }
      }
      k.gate.w1 = upload_f32(m, f1.data(), f1.size());
      k.gate.b1 = upload_key(m, p + ".se.conv_reduce.bias");
      k.gate.w2t = upload_f32(m, f2t.data(), f2t.size());
      k.gate.b2 = upload_f32(m, fb2.data(), fb2.size());
    }
    k.g2 = gh_module(m, p + ".ghost2", false);
    k.has_sc = !(cin == r.cout && r.stride == 1);
    if (k.has_sc) {
      k.sc_dw = gh_dw(m, p + ".shortcut.0", p + ".shortcut.1", r.stride);
      k.sc_pw = gh_pw(m, p + ".shortcut.2", p + ".shortcut.3", false);
    }
    gh.blocks.push_back(k);
    cin = r.cout;
  }
  gh.head = gh_pw(m, b + "blocks.9.0.conv", b + "blocks.9.0.bn1", false);
  gh.last = gh_pw(m, b + "Conv3", b + "Bn3", false);
  return 0;
}

// GhostNetV2.forward (ghostnetv2.py:418-441) at input 256: stem -> raw (x0) and relu(bn1) (bufA), both
// [B][128][128][16]; Conv1 (2x2 mean folded in) over raw -> f0, Conv2 -> f1; the 16 blocks ping-pong bufA /
// bufB with a module's primary output in t1, ghost1's output in t2 and, in eighths of sc, the stride-2
// depthwise output (2), the pooled input, the DFC branch's 1x1 output, its gate, the shortcut's depthwise
// and 1x1 outputs; blocks.9.0 -> t2, Conv3 -> f2
int rt_backbone_ghostv2(spe_model* m, hipStream_t s, const ImageSrc& images, int B, char* ws, const RtWs& w) {
  const RtModel& r = *m->rt;
  const RtGhost& gh = r.gh;
  const int dt = r.cfg.dtype, S = r.cfg.input_size;
  const double E = m->esz;
  auto P = [&](size_t o) { return (void*)(ws + o); };
  const size_t eighth = (size_t)B * S * S * 2 * m->esz;      // of a `big` buffer: 131072 elements an image at 256
  const size_t sc_dw = w.sc, sc_pool = w.sc + 2 * eighth, sc_res = w.sc + 3 * eighth, sc_gate = w.sc + 4 * eighth,
               sc_sdw = w.sc + 5 * eighth, sc_spw = w.sc + 6 * eighth;
  auto fits = [&](size_t elems_per_image, size_t eighths) { return elems_per_image * B * m->esz <= eighths * eighth; };
  const MbRun x{m, s, B};
  // x1 (t1, [B][H][H][half_p]) -> out [B][H][H][2 half_p]
  auto cheap = [&](const GhModule& g, int H, void* outp, int act, int post, const void* gate, const void* resid, float* pool) {
    GhCheapArgs a{};
    a.x1 = P(w.t1); a.ldx = g.half_p; a.xoff = 0;
    a.w = g.cheap_w; a.bias = g.cheap_b; a.out = outp; a.gate = gate; a.resid = resid; a.pool = pool;
    a.B = B; a.H = H; a.W = H; a.half = g.half_p; a.act = act; a.post = post;
    const double px = (double)B * H * H * g.half_p;
    return run_other(m, "conv.ghost", 2.0 * px * 9, px * (3 + (post == GH_POST_RESIDUAL ? 2 : 0)) * E, s,
                     [&] { return spe_launch_gh_cheap(a, dt, s); });
  };
  const int H0 = S / 2;
  CK(run_other(m, "conv.stem.gh", 2.0 * B * H0 * H0 * 16 * 27,
               (double)B * (S * S * image_px_bytes(images) + 2.0 * H0 * H0 * 16 * E), s, [&] {
    return spe_launch_gh_stem(images, gh.stem_w, gh.stem_scale, gh.stem_shift, P(w.x0), P(w.bufA), B, S, dt, s);
  }));
  CK(mb_run_pw(x, gh.conv_b, P(w.x0), H0, P(w.f0), MB_ACT_HSWISH, nullptr, nullptr));
  CK(mb_run_pw(x, gh.conv_c, P(w.f0), r.lvl_s[0], P(w.f1), MB_ACT_HSWISH, nullptr, nullptr));
  int H = H0;
  size_t cur = w.bufA;
  for (const GhBlock& k : gh.blocks) {
    const int Ho = H / k.stride;
    const size_t outbuf = cur == w.bufA ? w.bufB : w.bufA;
    // t2 holds ghost1's output; the slices of sc hold what only some blocks make
    if (!fits((size_t)H * H * k.mid_p, 8) || (k.stride > 1 && !fits((size_t)Ho * Ho * k.mid_p, 2)) ||
        (k.g1.attn && !fits((size_t)(H / 2) * (H / 2) * (k.mid_p > k.cin_p ? k.mid_p : k.cin_p), 1)) ||
        (k.has_sc && (!fits((size_t)Ho * Ho * k.cout_p, 1) || !fits((size_t)Ho * Ho * k.cin_p, 1))))
      return fail(SPE_E_WORKSPACE, "GhostNetV2 block buffers exceed the plan");
    // ghost1: the DFC gate first (mode "attn"), then primary -> t1, cheap + gate -> t2
    const void* gate = nullptr;
    if (k.g1.attn) {
      const int Hp = H / 2;
      CK(run_other(m, "eltwise.pool2", 0.0, (double)B * k.cin_p * (H * H + Hp * Hp) * E, s,
                   [&] { return spe_launch_gh_pool2(P(cur), P(sc_pool), B, H, H, k.cin_p, dt, s); }));
      CK(mb_run_pw(x, k.g1.short_pw, P(sc_pool), Hp, P(sc_res), MB_ACT_NONE, nullptr, nullptr));
      GhDfcArgs a{};
      a.x = P(sc_res); a.gate = P(sc_gate);
      a.w1 = k.g1.dfc_w1; a.b1 = k.g1.dfc_b1; a.w2 = k.g1.dfc_w2; a.b2 = k.g1.dfc_b2;
      a.B = B; a.H = Hp; a.W = Hp; a.C = k.mid_p;
      CK(run_other(m, "conv.dfc", 2.0 * B * Hp * Hp * k.mid_p * 25, 2.0 * B * Hp * Hp * k.mid_p * E, s,
                   [&] { return spe_launch_gh_dfc(a, dt, s); }));
      gate = a.gate;
    }
    CK(mb_run_pw(x, k.g1.primary, P(cur), H, P(w.t1), MB_ACT_RELU, nullptr, nullptr));
    float* pool = nullptr;
    const int tiles = spe_mb_dwconv_tiles(Ho, Ho);      // gh_cheap tiles the same 8 x 8 grid
    if (k.se) {
      if ((size_t)tiles * k.mid_p > MB_POOL_MAX) return fail(SPE_E_WORKSPACE, "SE pool partials exceed the plan");
      pool = (float*)P(w.mbpool);
    }
    CK(cheap(k.g1, H, P(w.t2), MB_ACT_RELU, gate ? GH_POST_GATE : GH_POST_NONE, gate, nullptr, k.stride == 1 ? pool : nullptr));
    const void* mid = P(w.t2);
    if (k.stride > 1) {
      CK(mb_run_dw(x, k.dw, P(w.t2), H, P(sc_dw), MB_ACT_NONE, pool));
      mid = P(sc_dw);
    }
    const float* scale = nullptr;
    if (k.se) {
      CK(mb_run_se(x, k.gate, pool, tiles, Ho, k.mid_p, (float*)P(w.mbscale)));
      scale = (const float*)P(w.mbscale);
    }
    // shortcut, then ghost2: primary (SE scale on A) -> t1, cheap + residual -> the block's output
    const void* res = P(cur);
    if (k.has_sc) {
      CK(mb_run_dw(x, k.sc_dw, P(cur), H, P(sc_sdw), MB_ACT_NONE, nullptr));
      CK(mb_run_pw(x, k.sc_pw, P(sc_sdw), Ho, P(sc_spw), MB_ACT_NONE, nullptr, nullptr));
      res = P(sc_spw);
    }
    CK(mb_run_pw(x, k.g2.primary, mid, Ho, P(w.t1), MB_ACT_NONE, nullptr, scale));
    CK(cheap(k.g2, Ho, P(outbuf), MB_ACT_NONE, GH_POST_RESIDUAL, nullptr, res, nullptr));
    H = Ho;
    cur = outbuf;
  }
  CK(mb_run_pw(x, gh.head, P(cur), H, P(w.t2), MB_ACT_RELU, nullptr, nullptr));
  CK(mb_run_pw(x, gh.last, P(w.t2), H, P(w.f2), MB_ACT_HSWISH, nullptr, nullptr));
  return 0;
}

const char* ghost_refuses(const spe_rtdetr_config& c) {
  return c.input_size == 256 ? nullptr
                             : "GhostNetV2 supports input_size 256 only: the backbone resizes its raw stem output to a "
                               "hard-coded 64x64, which is the stride-4 grid the stride-8 / 16 levels are built from "
                               "only at 256";
}

}  // namespace

const RtBackbone* rt_bb_ghostv2() {
  static const RtBackbone bb = {
      [](const spe_rtdetr_config& c) { return c.depth == SPE_RTDETR_GHOSTNETV2; },
      ghost_refuses,
      [](const spe_rtdetr_config&, int fch[3]) { fch[0] = 128; fch[1] = 256; fch[2] = 512; },
      ghost_spec, build_ghost, rt_backbone_ghostv2, true};
  return &bb;
}

