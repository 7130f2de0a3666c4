// Native runtime of the UNC RT-DETR keypoint model: parameter space in the
// reference's state_dict order (spe/rtdetr_spec.py mirrors it and tests pin it to the reference
// model's own keys), BatchNorm folding and the inference-time reparameterisations the reference
// itself defines, workspace plan and the launch sequence of RTDETR.forward in eval
// (UNC/src/zoo/rtdetr/rtdetr.py:36-53):
//
//   PResNet-vd (UNC/nn/backbone/presnet.py:156-265) -> HybridEncoder (hybrid_encoder.py:332-401)
//   -> RTDETRTransformer (rtdetr_decoder.py:505-710) -> RTDETRPostProcessor
//      (rtdetr_postprocessor.py:44-76)
//
// Folds: every ConvNormLayer's eval BatchNorm into its conv; RepVggBlock's 3x3 + 1x1 branches
// into one 3x3 conv (RepVggBlock.convert_to_deploy, hybrid_encoder.py:55-95); the variant-d
// shortcut AvgPool2d(2, 2, ceil_mode) + 1x1 conv into one 2x2 stride-2 conv with w/4 per tap
// (exact for the even feature sizes of inputs that are multiples of 32).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "launch.h"
#include "model_state.h"
#include "registry.h"

#define fail spe_fail

namespace {

const int RESNET_CFG18[4] = {2, 2, 2, 2}, RESNET_CFG50[4] = {3, 4, 6, 3};

inline bool is_mbv3_small(const spe_rtdetr_config& c) { return c.depth == SPE_RTDETR_MBV3_SMALL; }
inline bool is_mbv3(const spe_rtdetr_config& c) { return c.depth == SPE_RTDETR_MBV3_LARGE || is_mbv3_small(c); }
inline bool is_ghost(const spe_rtdetr_config& c) { return c.depth == SPE_RTDETR_GHOSTNETV2; }
inline bool is_presnet(const spe_rtdetr_config& c) { return !is_mbv3(c) && !is_ghost(c); }
inline int resnet_expansion(const spe_rtdetr_config& c) { return is_presnet(c) && c.depth >= 50 ? 4 : 1; }

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
struct MbTable { const MbRow* rows; int n, last_in, head_in; };   // conv2's and linear3's input widths
inline MbTable mb_table(const spe_rtdetr_config& c) {
  return is_mbv3_small(c) ? MbTable{MBV3_SMALL, 11, 96, 576} : MbTable{MBV3_LARGE, 15, 160, 960};
}
inline int se_hidden(int c) { return c / 4 > 8 ? c / 4 : 8; }

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

std::vector<std::pair<std::string, std::vector<int64_t>>> rt_spec(const spe_rtdetr_config& c) {
  std::vector<std::pair<std::string, std::vector<int64_t>>> s;
  const int64_t d = 256, C = c.num_classes + 1;
  auto add = [&](const std::string& k, std::vector<int64_t> sh) { s.emplace_back(k, std::move(sh)); };
  auto bn = [&](const std::string& p, int64_t ch) {
    for (const char* n : {"weight", "bias", "running_mean", "running_var"}) add(p + "." + n, {ch});
  };
  auto cnl = [&](const std::string& p, int64_t cin, int64_t cout, int64_t k) {
    add(p + ".conv.weight", {cout, cin, k, k});
    bn(p + ".norm", cout);
  };
  auto lin = [&](const std::string& p, int64_t o, int64_t i) { add(p + ".weight", {o, i}); add(p + ".bias", {o}); };
  auto mlp = [&](const std::string& p, std::vector<int64_t> dims) {
    for (size_t j = 0; j + 1 < dims.size(); ++j) lin(p + ".layers." + std::to_string(j), dims[j + 1], dims[j]);
  };
  auto mha = [&](const std::string& p) {
    add(p + ".in_proj_weight", {3 * d, d});
    add(p + ".in_proj_bias", {3 * d});
    lin(p + ".out_proj", d, d);
  };
  add("temper_param", {1});
  if (is_mbv3(c)) {     // registration order of MobileNetV3_{Large,Small}.__init__ (mobilenetv3.py:136-173, 241-270)
    const std::string b = "backbone.";
    const MbTable t = mb_table(c);
    add(b + "conv1.weight", {16, 3, 3, 3});
    if (!is_mbv3_small(c)) { bn(b + "bn1", 16); bn(b + "Bn1", 128); bn(b + "Bn2", 256); }
    add(b + "Conv1.weight", {128, 16, 3, 3});
    add(b + "Conv2.weight", {256, 128, 3, 3});
    if (is_mbv3_small(c)) bn(b + "bn1", 16);       // Small: Conv1 / Conv2 are bare, bn1 is registered after them
    for (int i = 0; i < t.n; ++i) {
      const MbRow& r = t.rows[i];
      const std::string p = b + "bneck." + std::to_string(i);
      add(p + ".conv1.weight", {r.cexp, r.cin, 1, 1}); bn(p + ".bn1", r.cexp);
      add(p + ".conv2.weight", {r.cexp, 1, r.k, r.k}); bn(p + ".bn2", r.cexp);
      if (r.se) {
        const int64_t h = se_hidden(r.cexp);
        add(p + ".se.se.1.weight", {h, r.cexp, 1, 1}); bn(p + ".se.se.2", h);
        add(p + ".se.se.4.weight", {r.cexp, h, 1, 1});
      }
      add(p + ".conv3.weight", {r.cout, r.cexp, 1, 1}); bn(p + ".bn3", r.cout);
      if (r.stride == 1 && r.cin != r.cout) {
        add(p + ".skip.0.weight", {r.cout, r.cin, 1, 1}); bn(p + ".skip.1", r.cout);
      } else if (r.stride == 2 && r.cin != r.cout) {
        add(p + ".skip.0.weight", {r.cin, 1, 3, 3}); bn(p + ".skip.1", r.cin);
        add(p + ".skip.2.weight", {r.cout, r.cin, 1, 1}); add(p + ".skip.2.bias", {r.cout}); bn(p + ".skip.3", r.cout);
      } else if (r.stride == 2) {
        add(p + ".skip.0.weight", {r.cout, 1, 3, 3}); bn(p + ".skip.1", r.cout);
      }
    }
    add(b + "conv2.weight", {512, t.last_in, 1, 1}); bn(b + "bn2", 512);
    add(b + "linear3.weight", {1280, t.head_in}); bn(b + "bn3", 1280);     // built, never called
  }
  if (is_ghost(c)) {    // registration order of GhostNetV2.__init__ (ghostnetv2.py:331-387)
    const std::string b = "backbone.";
    bn(b + "Bn1", 128); bn(b + "Bn2", 256); bn(b + "Bn3", 512);
    add(b + "Conv1.weight", {128, 16, 3, 3});
    add(b + "Conv2.weight", {256, 128, 3, 3});
    add(b + "Conv3.weight", {512, 960, 1, 1});
    add(b + "conv_stem.weight", {16, 3, 3, 3});
    bn(b + "bn1", 16);
    auto ghost = [&](const std::string& p, int64_t cin, int64_t cout, bool attn) {
      const int64_t h = (cout + 1) / 2;
      add(p + ".primary_conv.0.weight", {h, cin, 1, 1}); bn(p + ".primary_conv.1", h);
      add(p + ".cheap_operation.0.weight", {h, 1, 3, 3}); bn(p + ".cheap_operation.1", h);
      if (attn) {
        add(p + ".short_conv.0.weight", {cout, cin, 1, 1}); bn(p + ".short_conv.1", cout);
        add(p + ".short_conv.2.weight", {cout, 1, 1, 5}); bn(p + ".short_conv.3", cout);
        add(p + ".short_conv.4.weight", {cout, 1, 5, 1}); bn(p + ".short_conv.5", cout);
      }
    };
    int64_t cin = 16;
    for (int i = 0; i < 16; ++i) {
      const GhRow& r = GHOSTV2[i];
      const std::string p = gh_key(r);
      ghost(p + ".ghost1", cin, r.mid, i >= GH_ATTN_FROM);
      if (r.stride > 1) { add(p + ".conv_dw.weight", {r.mid, 1, r.k, r.k}); bn(p + ".bn_dw", r.mid); }
      if (r.se) {
        const int64_t h = gh_se_hidden(r.mid);
        add(p + ".se.conv_reduce.weight", {h, r.mid, 1, 1}); add(p + ".se.conv_reduce.bias", {h});
        add(p + ".se.conv_expand.weight", {r.mid, h, 1, 1}); add(p + ".se.conv_expand.bias", {r.mid});
      }
      ghost(p + ".ghost2", r.mid, r.cout, false);
      if (!(cin == r.cout && r.stride == 1)) {
        add(p + ".shortcut.0.weight", {cin, 1, r.k, r.k}); bn(p + ".shortcut.1", cin);
        add(p + ".shortcut.2.weight", {r.cout, cin, 1, 1}); bn(p + ".shortcut.3", r.cout);
      }
      cin = r.cout;
    }
    add(b + "blocks.9.0.conv.weight", {960, 160, 1, 1}); bn(b + "blocks.9.0.bn1", 960);
    add(b + "conv_head.weight", {1280, 960, 1, 1}); add(b + "conv_head.bias", {1280});   // built, never called
    lin(b + "classifier", 1000, 1280);
  }
  const bool bott = is_presnet(c) && c.depth >= 50;
  const int64_t exp = bott ? 4 : 1;
  if (is_presnet(c)) {
  cnl("backbone.conv1.conv1_1", 3, 32, 3);
  cnl("backbone.conv1.conv1_2", 32, 32, 3);
  cnl("backbone.conv1.conv1_3", 32, 64, 3);
  const int* nb = bott ? RESNET_CFG50 : RESNET_CFG18;
  const int64_t widths[4] = {64, 128, 256, 512};
  int64_t cin = 64;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < nb[i]; ++j) {
      const std::string p = "backbone.res_layers." + std::to_string(i) + ".blocks." + std::to_string(j);
      const int64_t co = widths[i];
      const bool s2 = j == 0 && i > 0;
      auto shortcut = [&] { if (j == 0) cnl(s2 ? p + ".short.conv" : p + ".short", cin, co * exp, 1); };
      if (bott) {
        cnl(p + ".branch2a", cin, co, 1);
        cnl(p + ".branch2b", co, co, 3);
        cnl(p + ".branch2c", co, co * exp, 1);
        shortcut();
      } else {                       // BasicBlock registers `short` before its branches
        shortcut();
        cnl(p + ".branch2a", cin, co, 3);
        cnl(p + ".branch2b", co, co, 3);
      }
      cin = co * exp;
    }
  }
  const int NL = 3, NP = 4, H = 8, P = H * NL * NP;
  for (int l = 0; l < NL; ++l) cnl("decoder.input_proj." + std::to_string(l), d, d, 1);
  for (int i = 0; i < c.dec_layers; ++i) {
    const std::string p = "decoder.decoder.layers." + std::to_string(i);
    mha(p + ".self_attn");
    add(p + ".norm1.weight", {d}); add(p + ".norm1.bias", {d});
    lin(p + ".cross_attn.sampling_offsets", 2 * P, d);
    lin(p + ".cross_attn.attention_weights", P, d);
    lin(p + ".cross_attn.value_proj", d, d);
    lin(p + ".cross_attn.output_proj", d, d);
    add(p + ".norm2.weight", {d}); add(p + ".norm2.bias", {d});
    lin(p + ".linear1", c.dec_ff, d);
    lin(p + ".linear2", d, c.dec_ff);
    add(p + ".norm3.weight", {d}); add(p + ".norm3.bias", {d});
  }
  for (int i = 0; i < c.dec_layers; ++i) mlp("decoder.decoder.sigma_embed." + std::to_string(i), {d, d, d, 1});
  mlp("decoder.query_pos_head", {2, 2 * d, d});
  lin("decoder.enc_output.0", d, d);
  add("decoder.enc_output.1.weight", {d}); add("decoder.enc_output.1.bias", {d});
  lin("decoder.enc_score_head", C, d);
  mlp("decoder.enc_bbox_head", {d, d, d, 2});
  for (int i = 0; i < c.dec_layers; ++i) lin("decoder.dec_score_head." + std::to_string(i), C, d);
  for (int i = 0; i < c.dec_layers; ++i) mlp("decoder.dec_bbox_head." + std::to_string(i), {d, d, d, 2});
  const int64_t bc[3] = {128 * exp, 256 * exp, 512 * exp};
  for (int l = 0; l < 3; ++l) {
    add("encoder.input_proj." + std::to_string(l) + ".0.weight", {d, bc[l], 1, 1});
    bn("encoder.input_proj." + std::to_string(l) + ".1", d);
  }
  add("encoder.encoder_fusion_input.weight", {d, 3 * d, 1, 1});
  const std::string a = "encoder.encoder.0.layers.0";
  mha(a + ".self_attn");
  lin(a + ".linear1", c.enc_ff, d);
  lin(a + ".linear2", d, c.enc_ff);
  for (const char* n : {"norm1", "norm2"}) { add(a + "." + n + ".weight", {d}); add(a + "." + n + ".bias", {d}); }
  for (int i = 0; i < 2; ++i) cnl("encoder.lateral_convs." + std::to_string(i), d, d, 1);
  const int64_t h = c.csp_hidden;
  for (const char* blocks : {"fpn_blocks", "pan_blocks"})
    for (int i = 0; i < 2; ++i) {
      const std::string p = std::string("encoder.") + blocks + "." + std::to_string(i);
      cnl(p + ".conv1", 2 * d, h, 1);
      cnl(p + ".conv2", 2 * d, h, 1);
      cnl(p + ".bottlenecks.0.conv1", h, h, 3);
      cnl(p + ".bottlenecks.0.conv2", h, h, 1);
      if (h != d) cnl(p + ".conv3", h, d, 1);
    }
  return s;
}

// rows [r0, r0+n) of several [*, K] weights stacked into one linear (one GEMM for several heads)
Conv stack_linears(spe_model* m, const std::vector<std::pair<std::string, std::string>>& parts, int K) {
  std::vector<float> rows, bias;
  int N = 0;
  for (auto& pr : parts) {
    const auto& w = m->host[pr.first];
    const auto& b = m->host[pr.second];
    rows.insert(rows.end(), w.begin(), w.end());
    bias.insert(bias.end(), b.begin(), b.end());
    N += (int)b.size();
  }
  Conv c;
  c.N = N; c.K = K; c.Kpad = pad64(K); c.Cin = K;
  c.w = upload_rows(m, rows, N, K, c.Kpad);
  c.bias = upload_f32(m, bias.data(), bias.size());
  return c;
}

RtHead make_head(spe_model* m, const std::string& cls, const std::string& box, const std::string& sigma) {
  RtHead h;
  std::vector<std::pair<std::string, std::string>> first{{box + ".layers.0.weight", box + ".layers.0.bias"}};
  if (!sigma.empty()) first.emplace_back(sigma + ".layers.0.weight", sigma + ".layers.0.bias");
  h.h1 = stack_linears(m, first, 256);
  h.box1 = make_linear(m, box + ".layers.1.weight", box + ".layers.1.bias", 0, 256, 256);
  h.box_w2 = upload_key(m, box + ".layers.2.weight");
  h.box_b2 = upload_key(m, box + ".layers.2.bias");
  if (!sigma.empty()) {
    h.sig1 = make_linear(m, sigma + ".layers.1.weight", sigma + ".layers.1.bias", 0, 256, 256);
    h.sig_w2 = upload_key(m, sigma + ".layers.2.weight");
    h.sig_b2 = upload_key(m, sigma + ".layers.2.bias");
  }
  if (!cls.empty()) {
    h.cls_w = upload_key(m, cls + ".weight");
    h.cls_b = upload_key(m, cls + ".bias");
  }
  return h;
}

// HybridEncoder.build_2d_sincos_position_embedding (hybrid_encoder.py:306-330) for a w x h grid,
// [w*h][256] in the reference's flatten order (meshgrid(w, h, 'ij'): token t <-> (t / h, t % h))
std::vector<float> sincos_2d(int w, int h, int d) {
  const int pd = d / 4;
  std::vector<float> omega(pd), out((size_t)w * h * d);
  for (int i = 0; i < pd; ++i) omega[i] = 1.0f / std::pow(10000.0f, (float)i / (float)pd);
  for (int t = 0; t < w * h; ++t) {
    const float gw = (float)(t / h), gh = (float)(t % h);
    float* o = &out[(size_t)t * d];
    for (int i = 0; i < pd; ++i) {
      const float ow = gw * omega[i], oh = gh * omega[i];
      o[i] = std::sin(ow);
      o[pd + i] = std::cos(ow);
      o[2 * pd + i] = std::sin(oh);
      o[3 * pd + i] = std::cos(oh);
    }
  }
  return out;
}

// RTDETRTransformer._generate_anchors (rtdetr_decoder.py:577-611): per token (x+0.5)/W,
// (y+0.5)/H, logit, +inf outside (eps, 1 - eps)
std::vector<float> make_anchors(const RtModel& r) {
  std::vector<float> a;
  const float eps = 1e-2f;
  for (int l = 0; l < 3; ++l) {
    const int s = r.lvl_s[l];
    for (int y = 0; y < s; ++y)
      for (int x = 0; x < s; ++x) {
        const float ax = ((float)x + 0.5f) / (float)s, ay = ((float)y + 0.5f) / (float)s;
        const bool valid = ax > eps && ax < 1 - eps && ay > eps && ay < 1 - eps;
        a.push_back(valid ? std::log(ax / (1 - ax)) : INFINITY);
        a.push_back(valid ? std::log(ay / (1 - ay)) : INFINITY);
      }
  }
  return a;
}

RtCsp make_csp(spe_model* m, const std::string& p, int h) {
  RtCsp c;
  c.c1 = make_conv(m, p + ".conv1.conv.weight", p + ".conv1.norm", "", 0, 1, 0);
  c.c2 = make_conv(m, p + ".conv2.conv.weight", p + ".conv2.norm", "", 0, 1, 0);
  std::vector<float> w3, b3, w1, b1;
  fold_conv(m, p + ".bottlenecks.0.conv1.conv.weight", p + ".bottlenecks.0.conv1.norm", "", w3, b3);
  fold_conv(m, p + ".bottlenecks.0.conv2.conv.weight", p + ".bottlenecks.0.conv2.norm", "", w1, b1);
  for (int co = 0; co < h; ++co) {                    // pad the 1x1 branch into the 3x3 centre tap
    for (int ci = 0; ci < h; ++ci) w3[((size_t)co * h + ci) * 9 + 4] += w1[(size_t)co * h + ci];
    b3[co] += b1[co];
  }
  c.rep = pack_conv(m, w3, b3, h, h, 3, 3, 0, 1, 1);
  c.has_c3 = h != 256;
  if (c.has_c3) c.c3 = make_conv(m, p + ".conv3.conv.weight", p + ".conv3.norm", "", 0, 1, 0);
  return c;
}

// largest tiles x channels product of an SE block's pool partials (block 11: 4 tiles x 672 at 256 input)
constexpr size_t MB_POOL_MAX = 4096;

// ---- workspace plan
struct RtWs {
  size_t x0, bufA, bufB, t1, t2, sc, f0, f1, f2;
  size_t cat0, cat1, catp0, catp1, aqk, avt, aao, atmp, affn, aout;
  size_t x1, x2, y, inner1, p3, n4, n5;
  size_t mbpool, mbscale;      // MobileNetV3: dwconv pool partials [B][MB_POOL_MAX], SE scales [B][960]
  size_t mem, omem, elog, value;
  size_t topk, tgt, slog, sanc, refs, qh, qpos, hh1, hh2, dqk, dvt, dao, dtmp, t1d, t2d, soaw, dcr, dffn, hs, lgt;
  size_t total;
};

RtWs rt_plan(const spe_model* m, int B) {
  const RtModel& r = *m->rt;
  const auto& c = r.cfg;
  const size_t E = m->esz, S = c.input_size, Q = c.num_queries, L = r.L, BQ = (size_t)B * Q;
  const size_t s0 = r.lvl_s[0], s1 = r.lvl_s[1], s2 = r.lvl_s[2];
  const size_t exp = resnet_expansion(c);
  RtWs w{};
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~size_t(255); return o; };
  const size_t big = (size_t)B * S * S * 16 * E;     // stride 2 x 64 ch == stride 4 x 256 ch
  w.x0 = take((size_t)B * S * S * 8 * E);
  w.bufA = take(big); w.bufB = take(big); w.t1 = take(big); w.t2 = take(big); w.sc = take(big);
  w.f0 = take((size_t)B * s0 * s0 * 128 * exp * E);
  w.f1 = take((size_t)B * s1 * s1 * 256 * exp * E);
  w.f2 = take((size_t)B * s2 * s2 * 512 * exp * E);
  w.cat0 = take((size_t)B * s0 * s0 * 512 * E);
  w.cat1 = take((size_t)B * s1 * s1 * 512 * E);
  w.catp0 = take((size_t)B * s1 * s1 * 512 * E);
  w.catp1 = take((size_t)B * s2 * s2 * 512 * E);
  const size_t T2 = (size_t)B * s2 * s2;
  w.aqk = take(T2 * 512 * E); w.avt = take(T2 * 256 * E); w.aao = take(T2 * 256 * E); w.atmp = take(T2 * 256 * E);
  w.affn = take(T2 * c.enc_ff * E); w.aout = take(T2 * 256 * E);
  const size_t hmax = (size_t)B * s0 * s0 * c.csp_hidden * E;
  w.x1 = take(hmax); w.x2 = take(hmax); w.y = take(hmax);
  w.inner1 = take((size_t)B * s1 * s1 * 256 * E);
  w.p3 = take((size_t)B * s0 * s0 * 256 * E);
  w.n4 = take((size_t)B * s1 * s1 * 256 * E);
  w.n5 = take((size_t)B * s2 * s2 * 256 * E);
  // (zero bytes for PResNet handles: their plan is what it was)
  w.mbpool = take(r.mbv3 || r.ghost ? (size_t)B * MB_POOL_MAX * 4 : 0);
  w.mbscale = take(r.mbv3 || r.ghost ? (size_t)B * 960 * 4 : 0);
  w.mem = take((size_t)B * L * 256 * E);
  w.omem = take((size_t)B * L * 256 * E);
  w.elog = take((size_t)B * L * (c.num_classes + 1) * 4);
  w.value = take((size_t)B * L * 256 * c.dec_layers * E);
  w.topk = take(BQ * 4);
  w.tgt = take(BQ * 256 * E);
  w.hh1 = take(BQ * 512 * E); w.hh2 = take(BQ * 512 * E);
  w.slog = take(BQ * (c.num_classes + 1) * 4); w.sanc = take(BQ * 2 * 4);
  w.refs = take((size_t)(c.dec_layers + 1) * BQ * 2 * 4);
  w.qh = take(BQ * 512 * E); w.qpos = take(BQ * 256 * E);
  w.dqk = take(BQ * 512 * E); w.dvt = take(BQ * 256 * E); w.dao = take(BQ * 256 * E); w.dtmp = take(BQ * 256 * E);
  w.t1d = take(BQ * 256 * E); w.t2d = take(BQ * 256 * E);
  w.soaw = take(BQ * 288 * 4); w.dcr = take(BQ * 256 * E); w.dffn = take(BQ * c.dec_ff * E);
  w.hs = take(BQ * 256 * 4);
  w.lgt = take(BQ * (c.num_classes + 1) * 4);
  w.total = off;
  return w;
}

// ---- MobileNetV3_Large packing: eval BatchNorm (eps 1e-5) folded in double, like fold_conv
void bn_fold(spe_model* m, const std::string& bn, int C, std::vector<double>& scale, std::vector<double>& shift) {
  scale.assign(C, 1.0);
  shift.assign(C, 0.0);
  if (bn.empty()) return;            // a bare conv (MobileNetV3_Small's Conv1 / Conv2): identity
  const auto& g = m->host[bn + ".weight"];
  const auto& b = m->host[bn + ".bias"];
  const auto& rm = m->host[bn + ".running_mean"];
  const auto& rv = m->host[bn + ".running_var"];
  for (int c = 0; c < C; ++c) {
    scale[c] = (double)g[c] / std::sqrt((double)rv[c] + 1e-5);
    shift[c] = (double)b[c] - (double)rm[c] * scale[c];
  }
}

// conv [cout][cin][kh][kw] (+ a bias in front of the norm) + BatchNorm -> rows [cout][(y*kw + x)*cin + ci]
// (the plain tap-major K order mb_gemm's A loader walks), folded bias.  pool2: the conv reads a 2x2 mean
// of its input -- folded into a (2kh)x(2kw) kernel of stride 2*stride, pad 2*pad, w/4 per tap (exact).
Conv mb_conv(spe_model* m, const std::string& wkey, const std::string& bn, const std::string& biaskey, int stride,
             int pad, bool pool2 = false) {
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
  Conv c;
  c.N = cout; c.K = K; c.Kpad = pad64(K); c.Cin = cin; c.KH = KH; c.KW = KW; c.stride = stride * f; c.pad = pad * f;
  c.w = upload_rows(m, rows, c.N, c.K, c.Kpad);
  c.bias = upload_f32(m, bias.data(), bias.size());
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

void build_mbv3(spe_model* m) {
  RtMbv3& mb = m->rt->mb;
  const std::string b = "backbone.";
  const bool small = m->rt->mb_small;
  const MbTable tab = mb_table(m->rt->cfg);
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
      k.se_hidden = h;
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
      k.se_w1 = upload_f32(m, f1.data(), f1.size());
      k.se_b1 = upload_f32(m, b1.data(), b1.size());
      k.se_w2t = upload_f32(m, f2t.data(), f2t.size());
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
}

// bytes a backbone's first launch reads per input pixel: the fp32 batch's three channels or the crop's 1 / 3
inline double image_px_bytes(const ImageSrc& img) { return img.u8 ? (double)img.ch : 12.0; }

// ---- backbone stages: both leave f0 / f1 / f2 (NHWC, strides 8 / 16 / 32) where the hybrid encoder reads them
int rt_backbone_presnet(spe_model* m, hipStream_t s, const ImageSrc& images, int B, char* ws, const RtWs& w) {
  const RtModel& r = *m->rt;
  const auto& c = r.cfg;
  const int dt = c.dtype, S = c.input_size, E = m->esz;
  auto P = [&](size_t o) { return (void*)(ws + o); };
  // conv as an implicit GEMM, or a plain GEMM over NHWC rows when it is 1x1 / stride 1; the
  // residual R (same row layout as the output) is added before the activation
  auto cgemm = [&](const char* kind, const Conv& cv, const void* in, int Hin, void* outp, int ldc, int act,
                   const void* R) {
    GemmArgs g;
    int mode = GEMM_CONV;
    if (cv.KH == 1 && cv.KW == 1 && cv.stride == 1 && cv.pad == 0) {
      g = linear_args(cv, in, cv.Cin, B * Hin * Hin, outp, ldc);
      mode = GEMM_LINEAR;
    } else {
      g = conv_args(cv, in, B, Hin, Hin, outp, ldc);
    }
    g.act = act;
    g.R = R; g.ldr = ldc;
    return run_gemm(m, kind, g, mode, s);
  };

  // ---------------- PResNet-vd (presnet.py:248-265)
  CK(run_other(m, "eltwise.pack", 0.0, (double)B * S * S * (image_px_bytes(images) + 8 * E), s,
               [&] { return spe_launch_pack_input(images, P(w.x0), B, S, dt, s); }));
  int H = S;
  size_t cur = w.x0;
  const size_t stem_out[3] = {w.bufA, w.bufB, w.bufA};
  for (int i = 0; i < 3; ++i) {
    GemmArgs g = conv_args(r.stem[i], P(cur), B, H, H, P(stem_out[i]), r.stem[i].N);
    g.act = ACT_RELU;
    CK(run_gemm(m, "rt.conv.stem", g, GEMM_CONV, s));
    H = g.Ho;
    cur = stem_out[i];
  }
  const int Hp = (H + 2 - 3) / 2 + 1;
  CK(run_other(m, "eltwise.maxpool", 0.0, (double)B * 64 * (H * H + Hp * Hp) * E, s,
               [&] { return spe_launch_maxpool3s2(P(cur), P(w.bufB), B, H, H, 64, Hp, Hp, dt, s); }));
  H = Hp;
  cur = w.bufB;
  const size_t feat[3] = {w.f0, w.f1, w.f2};
  for (int st = 0; st < 4; ++st)
    for (int j = 0; j < r.stage_n[st]; ++j) {
      const RtBlock& b = r.blocks[r.stage_first[st] + j];
      const int Ho = H / b.stride;
      const bool last = j == r.stage_n[st] - 1;
      const size_t outbuf = (last && st > 0) ? feat[st - 1] : (cur == w.bufA ? w.bufB : w.bufA);
      size_t res = cur;
      if (b.has_sc) {
        CK(cgemm(b.stride == 2 ? "rt.conv.short" : "rt.conv.1x1", b.sc, P(cur), H, P(w.sc), b.cout, ACT_NONE, nullptr));
        res = w.sc;
      }
      CK(cgemm(b.bottleneck ? "rt.conv.1x1" : "rt.conv.3x3", b.a, P(cur), H, P(w.t1), b.a.N, ACT_RELU, nullptr));
      const int Ha = (H + 2 * b.a.pad - b.a.KH) / b.a.stride + 1;
      if (b.bottleneck) {
        CK(cgemm("rt.conv.3x3", b.b, P(w.t1), Ha, P(w.t2), b.b.N, ACT_RELU, nullptr));
        CK(cgemm("rt.conv.1x1", b.c, P(w.t2), Ho, P(outbuf), b.cout, ACT_RELU, P(res)));
      } else {
        CK(cgemm("rt.conv.3x3", b.b, P(w.t1), Ha, P(outbuf), b.cout, ACT_RELU, P(res)));
      }
      H = Ho;
      cur = outbuf;
    }
  return 0;
}

// MobileNetV3_Large.forward / MobileNetV3_Small.forward (mobilenetv3.py:206-225, 301-320) at input 256: stem -> x0 [B][128][128][16]; Conv1 (2x2
// mean folded in) -> f0, Conv2 -> f1; the 15 blocks ping-pong bufA / bufB with the expanded tensor in t1,
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
  // 1x1 conv (or Conv1 / Conv2's implicit GEMM) over an NHWC map of edge Hin
  auto pw = [&](const Conv& cv, const void* in, int Hin, void* outp, int act, const void* R, const float* scale) {
    MbGemmArgs g{};
    const int Ho = (Hin + 2 * cv.pad - cv.KH) / cv.stride + 1;
    g.A = in; g.lda = cv.Cin;
    g.Bw = cv.w; g.ldb = cv.Kpad;
    g.bias = cv.bias; g.scale = scale;
    g.R = R; g.ldr = cv.N;
    g.C = outp; g.ldc = cv.N;
    g.M = B * Ho * Ho; g.N = cv.N; g.K = cv.K;
    g.H = Hin; g.W = Hin; g.Cin = cv.Cin; g.KH = cv.KH; g.KW = cv.KW; g.stride = cv.stride; g.pad = cv.pad;
    g.Ho = Ho; g.Wo = Ho;
    g.act = act;
    const double a_elems = (double)B * Hin * Hin * cv.Cin;
    return run_other(m, "conv.pw.mb", 2.0 * g.M * g.N * g.K,
                     (a_elems + (double)g.N * g.K + (double)g.M * g.N * (R ? 2 : 1)) * E, s,
                     [&] { return spe_launch_mb_gemm(g, dt, s); });
  };
  auto dw = [&](const MbDw& d, const void* in, int Hin, void* outp, int act, float* pool) {
    MbDwArgs a{};
    a.in = in; a.out = outp; a.w = d.w; a.bias = d.bias; a.pool = pool;
    a.B = B; a.H = Hin; a.W = Hin; a.C = d.C; a.k = d.k; a.stride = d.stride; a.act = act;
    const int Ho = Hin / d.stride;
    return run_other(m, "conv.dw", 2.0 * B * Ho * Ho * d.C * d.k * d.k,
                     (double)B * d.C * (Hin * Hin + Ho * Ho) * E, s, [&] { return spe_launch_mb_dwconv(a, dt, s); });
  };
  const int H0 = S / 2;
  const bool fused = r.mb_small && spe_mbs_entry_enabled();
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
    CK(pw(mb.conv_b3, P(w.x0), S / 4, P(w.f0), mb.side_act, nullptr, nullptr));
  } else {
    CK(run_other(m, "conv.stem.mb", 2.0 * B * H0 * H0 * 16 * 27,
                 (double)B * (S * S * image_px_bytes(images) + H0 * H0 * 16 * E), s,
                 [&] { return spe_launch_mb_stem(images, mb.stem_w, mb.stem_b, P(w.x0), B, S, dt, s); }));
    CK(pw(mb.conv_b, P(w.x0), H0, P(w.f0), mb.side_act, nullptr, nullptr));
  }
  CK(pw(mb.conv_c, P(w.f0), r.lvl_s[0], P(w.f1), mb.side_act, nullptr, nullptr));
  int H = H0;
  size_t cur = w.x0;
  const size_t sc_pw = w.sc + (((w.f0 - w.sc) / 2) & ~size_t(255));   // second half of sc: the skip branch's 1x1 output
  bool entry_done = fused;             // block 0's expand, depthwise and skip are already in t2 / sc
  for (const MbBlock& k : mb.blocks) {
    const int Ho = H / k.stride;
    const size_t outbuf = cur == w.bufA ? w.bufB : w.bufA;
    const bool head = entry_done;
    entry_done = false;
    if (!head) CK(pw(k.expand, P(cur), H, P(w.t1), k.act, nullptr, nullptr));
    float* pool = nullptr;
    const int tiles = spe_mb_dwconv_tiles(Ho, Ho);
    if (k.se) {
      if ((size_t)tiles * k.cexp > MB_POOL_MAX) return fail(SPE_E_WORKSPACE, "SE pool partials exceed the plan");
      pool = (float*)P(w.mbpool);      // rows [B][tiles][C]: B * tiles * C <= B * MB_POOL_MAX floats
    }
    if (!head) CK(dw(k.dw, P(w.t1), H, P(w.t2), k.act, pool));
    const float* scale = nullptr;
    if (k.se) {
      MbSeArgs a{};
      a.pool = pool; a.tiles = tiles; a.inv_hw = 1.0f / (float)(Ho * Ho);
      a.w1 = k.se_w1; a.b1 = k.se_b1; a.w2t = k.se_w2t;
      a.scale = (float*)P(w.mbscale);
      a.B = B; a.C = k.cexp; a.hidden = k.se_hidden;
      CK(run_other(m, "rt.se", 4.0 * B * k.cexp * k.se_hidden, ((double)B * (tiles + 1) * k.cexp + 2.0 * k.cexp * k.se_hidden) * 4, s,
                   [&] { return spe_launch_mb_se_gate(a, s); }));
      scale = a.scale;
    }
    const void* res = P(cur);
    if (k.has_skip_dw) {
      if (!head) CK(dw(k.skip_dw, P(cur), H, P(w.sc), MB_ACT_NONE, nullptr));
      res = P(w.sc);
    }
    if (k.has_skip_pw) {
      CK(pw(k.skip_pw, res, k.has_skip_dw ? Ho : H, P(sc_pw), MB_ACT_NONE, nullptr, nullptr));
      res = P(sc_pw);
    }
    CK(pw(k.project, P(w.t2), Ho, P(outbuf), k.act, res, scale));
    H = Ho;
    cur = outbuf;
  }
  CK(pw(mb.last, P(cur), H, P(w.f2), MB_ACT_HSWISH, nullptr, nullptr));
  return 0;
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
  Conv c;
  c.N = N; c.K = K; c.Kpad = pad64(K); c.Cin = K; c.KH = 1; c.KW = 1; c.stride = 1; c.pad = 0;
  c.w = upload_rows(m, rows, c.N, c.K, c.Kpad);
  c.bias = upload_f32(m, bias.data(), bias.size());
  return c;
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

void build_ghost(spe_model* m) {
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
      k.se_hidden = h;
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
      k.se_w1 = upload_f32(m, f1.data(), f1.size());
      k.se_b1 = upload_key(m, p + ".se.conv_reduce.bias");
      k.se_w2t = upload_f32(m, f2t.data(), f2t.size());
      k.se_b2 = upload_f32(m, fb2.data(), fb2.size());
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
  auto pw = [&](const Conv& cv, const void* in, int Hin, void* outp, int act, const float* scale) {
    MbGemmArgs g{};
    const int Ho = (Hin + 2 * cv.pad - cv.KH) / cv.stride + 1;
    g.A = in; g.lda = cv.Cin;
    g.Bw = cv.w; g.ldb = cv.Kpad;
    g.bias = cv.bias; g.scale = scale;
    g.C = outp; g.ldc = cv.N;
    g.M = B * Ho * Ho; g.N = cv.N; g.K = cv.K;
    g.H = Hin; g.W = Hin; g.Cin = cv.Cin; g.KH = cv.KH; g.KW = cv.KW; g.stride = cv.stride; g.pad = cv.pad;
    g.Ho = Ho; g.Wo = Ho;
    g.act = act;
    return run_other(m, "conv.pw.mb", 2.0 * g.M * g.N * g.K,
                     ((double)B * Hin * Hin * cv.Cin + (double)g.N * g.K + (double)g.M * g.N) * E, s,
                     [&] { return spe_launch_mb_gemm(g, dt, s); });
  };
  auto dw = [&](const MbDw& d, const void* in, int Hin, void* outp, float* pool) {
    MbDwArgs a{};
    a.in = in; a.out = outp; a.w = d.w; a.bias = d.bias; a.pool = pool;
    a.B = B; a.H = Hin; a.W = Hin; a.C = d.C; a.k = d.k; a.stride = d.stride; a.act = MB_ACT_NONE;
    const int Ho = Hin / d.stride;
    return run_other(m, "conv.dw", 2.0 * B * Ho * Ho * d.C * d.k * d.k,
                     (double)B * d.C * (Hin * Hin + Ho * Ho) * E, s, [&] { return spe_launch_mb_dwconv(a, dt, s); });
  };
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
  CK(pw(gh.conv_b, P(w.x0), H0, P(w.f0), MB_ACT_HSWISH, nullptr));
  CK(pw(gh.conv_c, P(w.f0), r.lvl_s[0], P(w.f1), MB_ACT_HSWISH, nullptr));
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
      CK(pw(k.g1.short_pw, P(sc_pool), Hp, P(sc_res), MB_ACT_NONE, nullptr));
      GhDfcArgs a{};
      a.x = P(sc_res); a.gate = P(sc_gate);
      a.w1 = k.g1.dfc_w1; a.b1 = k.g1.dfc_b1; a.w2 = k.g1.dfc_w2; a.b2 = k.g1.dfc_b2;
      a.B = B; a.H = Hp; a.W = Hp; a.C = k.mid_p;
      CK(run_other(m, "conv.dfc", 2.0 * B * Hp * Hp * k.mid_p * 25, 2.0 * B * Hp * Hp * k.mid_p * E, s,
                   [&] { return spe_launch_gh_dfc(a, dt, s); }));
      gate = a.gate;
    }
    CK(pw(k.g1.primary, P(cur), H, P(w.t1), MB_ACT_RELU, nullptr));
    float* pool = nullptr;
    const int tiles = spe_mb_dwconv_tiles(Ho, Ho);      // gh_cheap tiles the same 8 x 8 grid
    if (k.se) {
      if ((size_t)tiles * k.mid_p > MB_POOL_MAX) return fail(SPE_E_WORKSPACE, "SE pool partials exceed the plan");
      pool = (float*)P(w.mbpool);
    }
    CK(cheap(k.g1, H, P(w.t2), MB_ACT_RELU, gate ? GH_POST_GATE : GH_POST_NONE, gate, nullptr, k.stride == 1 ? pool : nullptr));
    const void* mid = P(w.t2);
    if (k.stride > 1) {
      CK(dw(k.dw, P(w.t2), H, P(sc_dw), pool));
      mid = P(sc_dw);
    }
    const float* scale = nullptr;
    if (k.se) {
      MbSeArgs a{};
      a.pool = pool; a.tiles = tiles; a.inv_hw = 1.0f / (float)(Ho * Ho);
      a.w1 = k.se_w1; a.b1 = k.se_b1; a.w2t = k.se_w2t; a.b2 = k.se_b2;
      a.scale = (float*)P(w.mbscale);
      a.B = B; a.C = k.mid_p; a.hidden = k.se_hidden;
      CK(run_other(m, "rt.se", 4.0 * B * k.mid_p * k.se_hidden, ((double)B * (tiles + 1) * k.mid_p + 2.0 * k.mid_p * k.se_hidden) * 4, s,
                   [&] { return spe_launch_mb_se_gate(a, s); }));
      scale = a.scale;
    }
    // shortcut, then ghost2: primary (SE scale on A) -> t1, cheap + residual -> the block's output
    const void* res = P(cur);
    if (k.has_sc) {
      CK(dw(k.sc_dw, P(cur), H, P(sc_sdw), nullptr));
      CK(pw(k.sc_pw, P(sc_sdw), Ho, P(sc_spw), MB_ACT_NONE, nullptr));
      res = P(sc_spw);
    }
    CK(pw(k.g2.primary, mid, Ho, P(w.t1), MB_ACT_NONE, scale));
    CK(cheap(k.g2, Ho, P(outbuf), MB_ACT_NONE, GH_POST_RESIDUAL, nullptr, res, nullptr));
    H = Ho;
    cur = outbuf;
  }
  CK(pw(gh.head, P(cur), H, P(w.t2), MB_ACT_RELU, nullptr));
  CK(pw(gh.last, P(w.t2), H, P(w.f2), MB_ACT_HSWISH, nullptr));
  return 0;
}

}  // namespace

int spe_rtdetr_build_device(spe_model* m) {
  RtModel& r = *m->rt;
  const auto& c = r.cfg;
  const int d = 256;
  r.blocks.clear();
  if (r.mbv3 || r.ghost) {
    if (r.ghost) build_ghost(m);
    else build_mbv3(m);
    r.fch[0] = 128; r.fch[1] = 256; r.fch[2] = 512;
  } else {
  const std::string bb = "backbone.conv1.conv1_";
  r.stem[0] = make_conv(m, bb + "1.conv.weight", bb + "1.norm", "", 8, 2, 1);
  r.stem[1] = make_conv(m, bb + "2.conv.weight", bb + "2.norm", "", 0, 1, 1);
  r.stem[2] = make_conv(m, bb + "3.conv.weight", bb + "3.norm", "", 0, 1, 1);
  const bool bott = c.depth >= 50;
  const int* nb = bott ? RESNET_CFG50 : RESNET_CFG18;
  const int widths[4] = {64, 128, 256, 512}, exp = bott ? 4 : 1;
  int cin = 64;
  for (int i = 0; i < 4; ++i) {
    r.stage_first[i] = (int)r.blocks.size();
    r.stage_n[i] = nb[i];
    for (int j = 0; j < nb[i]; ++j) {
      const std::string p = "backbone.res_layers." + std::to_string(i) + ".blocks." + std::to_string(j);
      RtBlock b;
      b.bottleneck = bott;
      b.stride = (j == 0 && i > 0) ? 2 : 1;
      b.cin = cin;
      b.cout = widths[i] * exp;
      if (bott) {
        b.a = make_conv(m, p + ".branch2a.conv.weight", p + ".branch2a.norm", "", 0, 1, 0);
        b.b = make_conv(m, p + ".branch2b.conv.weight", p + ".branch2b.norm", "", 0, b.stride, 1);
        b.c = make_conv(m, p + ".branch2c.conv.weight", p + ".branch2c.norm", "", 0, 1, 0);
      } else {
        b.a = make_conv(m, p + ".branch2a.conv.weight", p + ".branch2a.norm", "", 0, b.stride, 1);
        b.b = make_conv(m, p + ".branch2b.conv.weight", p + ".branch2b.norm", "", 0, 1, 1);
      }
      if (j == 0) {
        b.has_sc = true;
        if (b.stride == 2) {     // AvgPool2d(2, 2, ceil_mode) + ConvNormLayer(1x1) == 2x2/2 conv, w/4 per tap
          std::vector<float> w1, bias;
          fold_conv(m, p + ".short.conv.conv.weight", p + ".short.conv.norm", "", w1, bias);
          std::vector<float> w4((size_t)b.cout * cin * 4);
          for (size_t k = 0; k < (size_t)b.cout * cin; ++k)
            for (int t = 0; t < 4; ++t) w4[k * 4 + t] = w1[k] * 0.25f;
          b.sc = pack_conv(m, w4, bias, b.cout, cin, 2, 2, 0, 2, 0);
        } else {
          b.sc = make_conv(m, p + ".short.conv.weight", p + ".short.norm", "", 0, 1, 0);
        }
      }
      r.blocks.push_back(b);
      cin = b.cout;
    }
  }
  for (int l = 0; l < 3; ++l) r.fch[l] = r.blocks[r.stage_first[l + 1]].cout;
  }
  for (int l = 0; l < 3; ++l) {
    const std::string p = "encoder.input_proj." + std::to_string(l);
    r.in_proj[l] = make_conv(m, p + ".0.weight", p + ".1", "", 0, 1, 0);
  }
  const std::string a = "encoder.encoder.0.layers.0";
  r.aqk = make_linear(m, a + ".self_attn.in_proj_weight", a + ".self_attn.in_proj_bias", 0, 2 * d, d);
  r.av = make_linear(m, a + ".self_attn.in_proj_weight", a + ".self_attn.in_proj_bias", 2 * d, d, d);
  r.ao = make_linear(m, a + ".self_attn.out_proj.weight", a + ".self_attn.out_proj.bias", 0, d, d);
  r.al1 = make_linear(m, a + ".linear1.weight", a + ".linear1.bias", 0, c.enc_ff, d);
  r.al2 = make_linear(m, a + ".linear2.weight", a + ".linear2.bias", 0, d, c.enc_ff);
  r.an1g = upload_key(m, a + ".norm1.weight"); r.an1b = upload_key(m, a + ".norm1.bias");
  r.an2g = upload_key(m, a + ".norm2.weight"); r.an2b = upload_key(m, a + ".norm2.bias");
  r.aifi_pos = upload_T(m, sincos_2d(r.lvl_s[2], r.lvl_s[2], d));
  for (int i = 0; i < 2; ++i) {
    const std::string p = "encoder.lateral_convs." + std::to_string(i);
    r.lateral[i] = make_conv(m, p + ".conv.weight", p + ".norm", "", 0, 1, 0);
  }
  for (int i = 0; i < 2; ++i) {
    r.fpn[i] = make_csp(m, "encoder.fpn_blocks." + std::to_string(i), c.csp_hidden);
    r.pan[i] = make_csp(m, "encoder.pan_blocks." + std::to_string(i), c.csp_hidden);
  }
  for (int l = 0; l < 3; ++l) {
    const std::string p = "decoder.input_proj." + std::to_string(l);
    r.dec_in[l] = make_conv(m, p + ".conv.weight", p + ".norm", "", 0, 1, 0);
  }
  r.enc_out = make_linear(m, "decoder.enc_output.0.weight", "decoder.enc_output.0.bias", 0, d, d);
  r.eo_g = upload_key(m, "decoder.enc_output.1.weight");
  r.eo_b = upload_key(m, "decoder.enc_output.1.bias");
  r.enc_score = make_linear(m, "decoder.enc_score_head.weight", "decoder.enc_score_head.bias", 0, c.num_classes + 1, d);
  std::vector<std::pair<std::string, std::string>> vp;
  for (int i = 0; i < c.dec_layers; ++i) {
    const std::string p = "decoder.decoder.layers." + std::to_string(i) + ".cross_attn.value_proj";
    vp.emplace_back(p + ".weight", p + ".bias");
  }
  r.vproj = stack_linears(m, vp, d);
  const auto anc = make_anchors(r);
  r.anchors = upload_f32(m, anc.data(), anc.size());
  r.enc_head = make_head(m, "", "decoder.enc_bbox_head", "");
  r.qp_w0 = upload_key(m, "decoder.query_pos_head.layers.0.weight");
  r.qp_b0 = upload_key(m, "decoder.query_pos_head.layers.0.bias");
  r.qp_l1 = make_linear(m, "decoder.query_pos_head.layers.1.weight", "decoder.query_pos_head.layers.1.bias", 0, d, 2 * d);
  r.dec.clear();
  for (int i = 0; i < c.dec_layers; ++i) {
    const std::string p = "decoder.decoder.layers." + std::to_string(i), is = std::to_string(i);
    RtDec e;
    e.sqk = make_linear(m, p + ".self_attn.in_proj_weight", p + ".self_attn.in_proj_bias", 0, 2 * d, d);
    e.sv = make_linear(m, p + ".self_attn.in_proj_weight", p + ".self_attn.in_proj_bias", 2 * d, d, d);
    e.so = make_linear(m, p + ".self_attn.out_proj.weight", p + ".self_attn.out_proj.bias", 0, d, d);
    e.soaw = stack_linears(m, {{p + ".cross_attn.sampling_offsets.weight", p + ".cross_attn.sampling_offsets.bias"},
                               {p + ".cross_attn.attention_weights.weight", p + ".cross_attn.attention_weights.bias"}}, d);
    e.oproj = make_linear(m, p + ".cross_attn.output_proj.weight", p + ".cross_attn.output_proj.bias", 0, d, d);
    e.l1 = make_linear(m, p + ".linear1.weight", p + ".linear1.bias", 0, c.dec_ff, d);
    e.l2 = make_linear(m, p + ".linear2.weight", p + ".linear2.bias", 0, d, c.dec_ff);
    e.n1g = upload_key(m, p + ".norm1.weight"); e.n1b = upload_key(m, p + ".norm1.bias");
    e.n2g = upload_key(m, p + ".norm2.weight"); e.n2b = upload_key(m, p + ".norm2.bias");
    e.n3g = upload_key(m, p + ".norm3.weight"); e.n3b = upload_key(m, p + ".norm3.bias");
    e.head = make_head(m, "decoder.dec_score_head." + is, "decoder.dec_bbox_head." + is, "decoder.decoder.sigma_embed." + is);
    r.dec.push_back(e);
  }
  return 0;
}

int64_t spe_rtdetr_workspace(const spe_model* m, int B) { return (int64_t)rt_plan(m, B).total; }

int spe_rtdetr_backbone(spe_model* m, hipStream_t s, const float* images, int B, void* workspace, int64_t ws_bytes,
                        const void** f, int* ch, int* hw) {
  if (!m || !workspace || !images || B <= 0) return fail(SPE_E_ARG, "bad argument");
  if (m->family != 1) return fail(SPE_E_ARG, "not an RT-DETR model");
  if (!m->finalized) return fail(SPE_E_STATE, "model not finalized");
  const RtWs w = rt_plan(m, B);
  if ((int64_t)w.total > ws_bytes) return fail(SPE_E_WORKSPACE, "workspace too small");
  const RtModel& r = *m->rt;
  char* ws = (char*)workspace;
  const ImageSrc src{images, nullptr, 0};
  CK(r.ghost ? rt_backbone_ghostv2(m, s, src, B, ws, w)
     : r.mbv3 ? rt_backbone_mbv3(m, s, src, B, ws, w) : rt_backbone_presnet(m, s, src, B, ws, w));
  const size_t off[3] = {w.f0, w.f1, w.f2};
  for (int l = 0; l < 3; ++l) {
    if (f) f[l] = ws + off[l];
    if (ch) ch[l] = r.fch[l];
    if (hw) hw[l] = r.lvl_s[l];
  }
  return 0;
}

extern "C" {

int spe_rtdetr_create(const spe_rtdetr_config* cfg, spe_model** out) {
  if (!cfg || !out) return fail(SPE_E_ARG, "null argument");
  if (cfg->depth != 18 && cfg->depth != 50 && !is_mbv3(*cfg) && !is_ghost(*cfg))
    return fail(SPE_E_ARG, "depth must be a PResNet depth (18 or 50), SPE_RTDETR_MBV3_LARGE, SPE_RTDETR_MBV3_SMALL or "
                           "SPE_RTDETR_GHOSTNETV2");
  if (is_ghost(*cfg) && cfg->input_size != 256)
    return fail(SPE_E_ARG, "GhostNetV2 supports input_size 256 only: the backbone resizes its raw stem output to a "
                           "hard-coded 64x64, which is the stride-4 grid the stride-8 / 16 levels are built from "
                           "only at 256");
  if (is_mbv3(*cfg) && cfg->input_size != 256)
    return fail(SPE_E_ARG, "MobileNetV3_Large / _Small support input_size 256 only: the backbone resizes its stem output to "
                           "a hard-coded 64x64, which is the stride-4 grid the stride-8 / 16 levels are built from "
                           "only at 256");
  if (cfg->input_size % 32 || cfg->input_size < 64) return fail(SPE_E_ARG, "input_size must be a multiple of 32, >= 64");
  if (cfg->num_queries < 1 || cfg->num_queries > 64) return fail(SPE_E_ARG, "num_queries must be in [1, 64]");
  if (cfg->dec_layers < 1 || cfg->enc_ff % 64 || cfg->dec_ff % 64 || cfg->csp_hidden % 64 || cfg->csp_hidden < 64 ||
      cfg->csp_hidden > 256 || cfg->num_classes < 1 || cfg->num_classes > 15)
    return fail(SPE_E_ARG, "bad RT-DETR configuration");
  if (cfg->dtype != SPE_DTYPE_BF16_ && cfg->dtype != SPE_DTYPE_F32_) return fail(SPE_E_ARG, "bad dtype");
  spe_model* m = new spe_model();
  m->family = 1;
  m->rt = new RtModel();
  m->rt->cfg = *cfg;
  m->rt->mbv3 = is_mbv3(*cfg);
  m->rt->mb_small = is_mbv3_small(*cfg);
  m->rt->ghost = is_ghost(*cfg);
  m->esz = cfg->dtype == SPE_DTYPE_BF16_ ? 2 : 4;
  m->cfg.dtype = cfg->dtype;
  m->cfg.input_size = cfg->input_size;
  m->cfg.num_queries = cfg->num_queries;
  m->spec = rt_spec(*cfg);
  RtModel& r = *m->rt;
  r.L = 0;
  for (int l = 0; l < 3; ++l) {
    r.lvl_s[l] = cfg->input_size >> (3 + l);
    r.lvl_start[l] = r.L;
    r.L += r.lvl_s[l] * r.lvl_s[l];
  }
  r.lvl_start[3] = r.L;
  if (cfg->num_queries > r.L) return (delete m->rt, delete m, fail(SPE_E_ARG, "num_queries exceeds the encoder tokens"));
  *out = m;
  return 0;
}

}  // extern "C"

namespace {

// One forward call's context: the stages below are the launch sequence of RTDETR.forward cut at the
// two points where everything the rest reads lies in the workspace (include/spe.h, staging contract).
struct RtFwd {
  spe_model* m;
  const RtWs& w;
  char* ws;
  hipStream_t s;
  int B;
  void* P(size_t o) const { return (void*)(ws + o); }
};

// TRANSFORMER: HybridEncoder (hybrid_encoder.py:332-401) over f0 / f1 / f2 -> p3 / n4 / n5
int rt_encoder_stage(const RtFwd& f) {
  spe_model* m = f.m;
  const RtWs& w = f.w;
  hipStream_t s = f.s;
  const int B = f.B;
  const RtModel& r = *m->rt;
  const auto& c = r.cfg;
  const int dt = c.dtype, d = 256, E = m->esz, h = c.csp_hidden;
  auto P = [&](size_t o) { return f.P(o); };
  const int s0 = r.lvl_s[0], s1 = r.lvl_s[1], s2 = r.lvl_s[2];
  const int* fch = r.fch;
  {  // input_proj (1x1 + BN): levels 0 / 1 straight into the second half of their FPN concat
    GemmArgs g0 = linear_args(r.in_proj[0], P(w.f0), fch[0], B * s0 * s0, (char*)P(w.cat0) + d * E, 2 * d);
    CK(run_gemm(m, "rt.enc.proj", g0, GEMM_LINEAR, s));
    GemmArgs g1 = linear_args(r.in_proj[1], P(w.f1), fch[1], B * s1 * s1, (char*)P(w.cat1) + d * E, 2 * d);
    CK(run_gemm(m, "rt.enc.proj", g1, GEMM_LINEAR, s));
    GemmArgs g2 = linear_args(r.in_proj[2], P(w.f2), fch[2], B * s2 * s2, P(w.aout), d);
    CK(run_gemm(m, "rt.enc.proj", g2, GEMM_LINEAR, s));
  }
  {  // AIFI: one post-norm transformer encoder layer on the stride-32 level (GELU FFN)
    const int T = s2 * s2, M = B * T;
    GemmArgs gq = linear_args(r.aqk, P(w.aout), d, M, P(w.aqk), 2 * d);
    gq.P = r.aifi_pos; gq.ldp = d; gq.prow = T;
    CK(run_gemm(m, "rt.aifi.qk", gq, GEMM_LINEAR_ADD, s));
    GemmArgs gv = linear_args(r.av, P(w.aout), d, M, P(w.avt), 8);
    gv.vt_T = T; gv.vt_B = B;
    CK(run_gemm(m, "rt.aifi.v", gv, GEMM_LINEAR, s));
    AttnArgs at{};
    at.q = P(w.aqk); at.ldq = 2 * d;
    at.k = (char*)P(w.aqk) + d * E; at.ldk = 2 * d;
    at.vt = P(w.avt);
    at.o = P(w.aao); at.ldo = d;
    at.B = B; at.H = 8; at.Tq = T; at.Tk = T; at.scale = 1.0f / std::sqrt(32.0f);
    CK(run_attn(m, "rt.attn.aifi", at, dt, s));
    GemmArgs go = linear_args(r.ao, P(w.aao), d, M, P(w.atmp), d);
    go.R = P(w.aout); go.ldr = d;
    CK(run_gemm(m, "rt.aifi.o", go, GEMM_LINEAR, s));
    CK(run_layernorm(m, "rt.ln", P(w.atmp), r.an1g, r.an1b, P(w.aout), nullptr, M, d, dt, s));
    GemmArgs g1 = linear_args(r.al1, P(w.aout), d, M, P(w.affn), c.enc_ff);
    g1.act = ACT_GELU;
    CK(run_gemm(m, "rt.aifi.ffn", g1, GEMM_LINEAR, s));
    GemmArgs g2 = linear_args(r.al2, P(w.affn), c.enc_ff, M, P(w.atmp), d);
    g2.R = P(w.aout); g2.ldr = d;
    CK(run_gemm(m, "rt.aifi.ffn", g2, GEMM_LINEAR, s));
    CK(run_layernorm(m, "rt.ln", P(w.atmp), r.an2g, r.an2b, P(w.aout), nullptr, M, d, dt, s));
  }
  // CSPRepLayer over a [rows][512] concat: conv1 / conv2 (1x1 + BN + SiLU), RepVGG 3x3 + SiLU + x2,
  // conv3 (1x1 + BN + SiLU) when hidden != 256
  auto csp = [&](const RtCsp& k, size_t in, int hw, size_t outb) -> int {
    const int M = B * hw * hw;
    GemmArgs g1 = linear_args(k.c1, P(in), 2 * d, M, P(w.x1), h);
    g1.act = ACT_SILU;
    int rc = run_gemm(m, "rt.csp.1x1", g1, GEMM_LINEAR, s);
    if (rc) return rc;
    GemmArgs g2 = linear_args(k.c2, P(in), 2 * d, M, P(w.x2), h);
    g2.act = ACT_SILU;
    if ((rc = run_gemm(m, "rt.csp.1x1", g2, GEMM_LINEAR, s))) return rc;
    GemmArgs g3 = conv_args(k.rep, P(w.x1), B, hw, hw, k.has_c3 ? P(w.y) : P(outb), h);
    g3.act = ACT_SILU; g3.R = P(w.x2); g3.ldr = h; g3.res_post = 1;
    if ((rc = run_gemm(m, "rt.csp.rep", g3, GEMM_CONV, s))) return rc;
    if (k.has_c3) {
      GemmArgs g4 = linear_args(k.c3, P(w.y), h, M, P(outb), d);
      g4.act = ACT_SILU;
      rc = run_gemm(m, "rt.csp.1x1", g4, GEMM_LINEAR, s);
    }
    return rc;
  };
  auto resample = [&](size_t in, int ldi, size_t outp, int hw, int mode) {
    return run_other(m, "rt.resample", 0.0, (double)B * hw * hw * d * E * (mode == 0 ? 5 : 1.25), s,
                     [&] { return spe_launch_resample2x(P(in), ldi, P(outp), 2 * d, B, hw, hw, d, mode, dt, s); });
  };
  {  // top-down FPN; each lateral output also lands in the second half of its PAN concat
    GemmArgs l0 = linear_args(r.lateral[0], P(w.aout), d, B * s2 * s2, (char*)P(w.catp1) + d * E, 2 * d);
    l0.act = ACT_SILU;
    CK(run_gemm(m, "rt.enc.lateral", l0, GEMM_LINEAR, s));
    CK(resample(w.catp1 + d * E, 2 * d, w.cat1, s2, 0));
    CK(csp(r.fpn[0], w.cat1, s1, w.inner1));
    GemmArgs l1 = linear_args(r.lateral[1], P(w.inner1), d, B * s1 * s1, (char*)P(w.catp0) + d * E, 2 * d);
    l1.act = ACT_SILU;
    CK(run_gemm(m, "rt.enc.lateral", l1, GEMM_LINEAR, s));
    CK(resample(w.catp0 + d * E, 2 * d, w.cat0, s1, 0));
    CK(csp(r.fpn[1], w.cat0, s0, w.p3));
  }
  {  // bottom-up PAN (bicubic x0.5)
    CK(run_other(m, "rt.resample", 0.0, (double)B * s0 * s0 * d * E * 1.25, s,
                 [&] { return spe_launch_resample2x(P(w.p3), d, P(w.catp0), 2 * d, B, s0, s0, d, 1, dt, s); }));
    CK(csp(r.pan[0], w.catp0, s1, w.n4));
    CK(run_other(m, "rt.resample", 0.0, (double)B * s1 * s1 * d * E * 1.25, s,
                 [&] { return spe_launch_resample2x(P(w.n4), d, P(w.catp1), 2 * d, B, s1, s1, d, 1, dt, s); }));
    CK(csp(r.pan[1], w.catp1, s2, w.n5));
  }
  return 0;
}

// DECODE: RTDETRTransformer (rtdetr_decoder.py:505-710), the heads and the fused RTDETRPostProcessor over
// p3 / n4 / n5 (everything else it reads it writes first)
int rt_decoder_stage(const RtFwd& f, const spe_rtdetr_outputs* out) {
  spe_model* m = f.m;
  const RtWs& w = f.w;
  hipStream_t s = f.s;
  const int B = f.B;
  const RtModel& r = *m->rt;
  const auto& c = r.cfg;
  const int dt = c.dtype, d = 256, Q = c.num_queries, C = c.num_classes + 1, E = m->esz;
  const int BQ = B * Q;
  auto P = [&](size_t o) { return f.P(o); };
  const size_t lvl_out[3] = {w.p3, w.n4, w.n5};
  for (int l = 0; l < 3; ++l) {   // level-major memory: rows [B * lvl_start[l] + b * hw_l + t]
    GemmArgs g = linear_args(r.dec_in[l], P(lvl_out[l]), d, B * r.lvl_s[l] * r.lvl_s[l],
                             (char*)P(w.mem) + (size_t)B * r.lvl_start[l] * d * E, d);
    CK(run_gemm(m, "rt.dec.proj", g, GEMM_LINEAR, s));
  }
  const int ML = B * r.L;
  {  // enc_output: Linear + LayerNorm
    GemmArgs g = linear_args(r.enc_out, P(w.mem), d, ML, P(w.omem), d);
    GemmArgs gf = g;
    gf.ln_g = r.eo_g; gf.ln_b = r.eo_b;
    if (E == 2 && spe_ln_fusable(gf)) {
      CK(run_gemm(m, "rt.dec.enc_out", gf, GEMM_LINEAR, s));
    } else {
      CK(run_gemm(m, "rt.dec.enc_out", g, GEMM_LINEAR, s));
      CK(run_layernorm(m, "rt.ln", P(w.omem), r.eo_g, r.eo_b, P(w.omem), nullptr, ML, d, dt, s));
    }
  }
  {
    GemmArgs g = linear_args(r.enc_score, P(w.omem), d, ML, P(w.elog), C);
    g.out_f32 = 1;
    CK(run_gemm(m, "rt.dec.enc_score", g, GEMM_LINEAR, s));
  }
  {  // every layer's value projection of the memory in one GEMM
    GemmArgs g = linear_args(r.vproj, P(w.mem), d, ML, P(w.value), r.vproj.N);
    CK(run_gemm(m, "rt.dec.value", g, GEMM_LINEAR, s));
  }
  RtSelectArgs sa{};
  sa.logits = (const float*)P(w.elog); sa.C = C;
  sa.memory = P(w.omem); sa.ldm = d;
  sa.anchors = r.anchors;
  sa.B = B; sa.Q = Q; sa.D = d; sa.levels = 3;
  for (int l = 0; l < 4; ++l) sa.lvl_start[l] = r.lvl_start[l];
  sa.topk = out->topk ? out->topk : (int*)P(w.topk);
  sa.target = P(w.tgt); sa.ldt = d;
  sa.sel_logits = out->enc_logits ? out->enc_logits : (float*)P(w.slog);
  sa.sel_anchors = (float*)P(w.sanc);
  CK(run_other(m, "rt.select", 0.0, (double)ML * C * 4, s, [&] { return spe_launch_query_select(sa, dt, s); }));
  // heads: the 256-wide hidden layers as GEMMs (box | sigma side by side), then head_finish
  auto heads = [&](const RtHead& k, const void* x, const float* hs32, RtHeadArgs ha) -> int {
    GemmArgs g1 = linear_args(k.h1, x, d, BQ, P(w.hh1), 2 * d);
    g1.act = ACT_RELU;
    int rc = run_gemm(m, "rt.heads", g1, GEMM_LINEAR, s);
    if (rc) return rc;
    GemmArgs g2 = linear_args(k.box1, P(w.hh1), 2 * d, BQ, P(w.hh2), 2 * d);
    g2.act = ACT_RELU;
    if ((rc = run_gemm(m, "rt.heads", g2, GEMM_LINEAR, s))) return rc;
    if (k.sig_w2) {
      GemmArgs g3 = linear_args(k.sig1, (char*)P(w.hh1) + d * E, 2 * d, BQ, (char*)P(w.hh2) + d * E, 2 * d);
      g3.act = ACT_RELU;
      if ((rc = run_gemm(m, "rt.heads", g3, GEMM_LINEAR, s))) return rc;
    }
    ha.rows = BQ; ha.Q = Q; ha.C = C;
    ha.hs = hs32; ha.cls_w = k.cls_w; ha.cls_b = k.cls_b;
    ha.h2 = P(w.hh2); ha.ld_h2 = 2 * d;
    ha.box_w2 = k.box_w2; ha.box_b2 = k.box_b2; ha.sig_w2 = k.sig_w2; ha.sig_b2 = k.sig_b2;
    return run_other(m, "rt.heads", 0.0, (double)BQ * d * 4, s, [&] { return spe_launch_head_finish(ha, dt, s); });
  };
  float* refs = (float*)P(w.refs);
  auto ref_buf = [&](int i) { return refs + (size_t)i * BQ * 2; };
  {  // initial reference points: sigmoid(enc_bbox_head(target) + anchors) (= enc_topk_bboxes)
    RtHeadArgs ha{};
    ha.pt_add = sa.sel_anchors; ha.pt_add_invsig = 0;
    ha.points = out->enc_points ? out->enc_points : ref_buf(0);
    CK(heads(r.enc_head, P(w.tgt), nullptr, ha));
    if (out->enc_points)
      CK((int)hipMemcpyAsync(ref_buf(0), out->enc_points, (size_t)BQ * 2 * 4, hipMemcpyDeviceToDevice, s));
  }
  size_t tgt = w.tgt;
  for (int i = 0; i < c.dec_layers; ++i) {
    const RtDec& e = r.dec[i];
    const bool last = i == c.dec_layers - 1;
    const float* ref = ref_buf(i);
    // query_pos_head(ref): relu(W0 ref + b0) (K = 2) -> Linear(512 -> 256)
    CK(run_other(m, "rt.qpos", 0.0, (double)BQ * 512 * E, s,
                 [&] { return spe_launch_qpos_hidden(ref, r.qp_w0, r.qp_b0, P(w.qh), BQ, 2 * d, dt, s); }));
    GemmArgs gp = linear_args(r.qp_l1, P(w.qh), 2 * d, BQ, P(w.qpos), d);
    CK(run_gemm(m, "rt.gemm.dec", gp, GEMM_LINEAR, s));
    // self-attention: q = k = tgt + qpos, v = tgt
    GemmArgs gq = linear_args(e.sqk, P(tgt), d, BQ, P(w.dqk), 2 * d);
    gq.P = P(w.qpos); gq.ldp = d; gq.prow = BQ;
    CK(run_gemm(m, "rt.gemm.dec", gq, GEMM_LINEAR_ADD, s));
    GemmArgs gv = linear_args(e.sv, P(tgt), d, BQ, P(w.dvt), 8);
    gv.vt_T = Q; gv.vt_B = B;
    CK(run_gemm(m, "rt.gemm.dec", gv, GEMM_LINEAR, s));
    AttnArgs at{};
    at.q = P(w.dqk); at.ldq = 2 * d;
    at.k = (char*)P(w.dqk) + d * E; at.ldk = 2 * d;
    at.vt = P(w.dvt);
    at.o = P(w.dao); at.ldo = d;
    at.B = B; at.H = 8; at.Tq = Q; at.Tk = Q; at.scale = 1.0f / std::sqrt(32.0f);
    CK(run_attn(m, "rt.attn.dec_self", at, dt, s));
    GemmArgs go = linear_args(e.so, P(w.dao), d, BQ, P(w.dtmp), d);
    go.R = P(tgt); go.ldr = d;
    CK(run_gemm(m, "rt.gemm.dec", go, GEMM_LINEAR, s));
    CK(run_layernorm(m, "rt.ln", P(w.dtmp), e.n1g, e.n1b, P(w.t1d), nullptr, BQ, d, dt, s));
    // multi-scale deformable cross-attention, query = tgt + qpos
    GemmArgs gs = linear_args(e.soaw, P(w.t1d), d, BQ, P(w.soaw), e.soaw.N);
    gs.P = P(w.qpos); gs.ldp = d; gs.prow = BQ; gs.out_f32 = 1;
    CK(run_gemm(m, "rt.gemm.dec", gs, GEMM_LINEAR_ADD, s));
    RtDeformArgs da{};
    da.value = (const char*)P(w.value) + (size_t)i * d * E; da.ldv = r.vproj.N;
    da.so_aw = (const float*)P(w.soaw); da.ld_so = e.soaw.N;
    da.ref = ref;
    da.out = P(w.dcr); da.ldo = d;
    da.rows = BQ; da.Q = Q; da.heads = 8; da.levels = 3; da.points = 4;
    for (int l = 0; l < 3; ++l) {
      da.lvl_h[l] = da.lvl_w[l] = r.lvl_s[l];
      da.lvl_rows0[l] = B * r.lvl_start[l];
    }
    CK(run_other(m, "rt.msdeform", 0.0, (double)BQ * 96 * 4 * 32 * E, s, [&] { return spe_launch_msdeform(da, dt, s); }));
    GemmArgs gc = linear_args(e.oproj, P(w.dcr), d, BQ, P(w.dtmp), d);
    gc.R = P(w.t1d); gc.ldr = d;
    CK(run_gemm(m, "rt.gemm.dec", gc, GEMM_LINEAR, s));
    CK(run_layernorm(m, "rt.ln", P(w.dtmp), e.n2g, e.n2b, P(w.t2d), nullptr, BQ, d, dt, s));
    // FFN (ReLU) + norm3
    GemmArgs g1 = linear_args(e.l1, P(w.t2d), d, BQ, P(w.dffn), c.dec_ff);
    g1.act = ACT_RELU;
    CK(run_gemm(m, "rt.gemm.dec", g1, GEMM_LINEAR, s));
    GemmArgs g2 = linear_args(e.l2, P(w.dffn), c.dec_ff, BQ, P(w.dtmp), d);
    g2.R = P(w.t2d); g2.ldr = d;
    CK(run_gemm(m, "rt.gemm.dec", g2, GEMM_LINEAR, s));
    tgt = (tgt == w.tgt) ? w.t1d : w.tgt;          // t1d is free again once the FFN residual is read
    CK(run_layernorm(m, "rt.ln", P(w.dtmp), e.n3g, e.n3b, P(tgt), (float*)P(w.hs), BQ, d, dt, s));
    // heads: score, refined points sigmoid(box MLP + inverse_sigmoid(ref)), sigma (+ PostProcess)
    RtHeadArgs ha{};
    ha.pt_add = ref; ha.pt_add_invsig = 1;
    const size_t aoff = (size_t)i * BQ;
    if (last) {
      ha.logits = out->logits; ha.points = out->points;
      ha.log_sigmas = out->log_sigmas;
      ha.clip_bbox = out->clip_bbox;
      ha.probs = out->clip_bbox ? out->probs : nullptr;
      ha.points_px = out->clip_bbox ? out->points_px : nullptr;
      ha.sigmas = out->clip_bbox ? out->sigmas : nullptr;
    } else {
      ha.logits = out->aux_logits ? out->aux_logits + aoff * C : (float*)P(w.lgt);
      ha.points = ref_buf(i + 1);
      ha.log_sigmas = out->aux_log_sigmas ? out->aux_log_sigmas + aoff * 2 : nullptr;
    }
    CK(heads(e.head, P(tgt), (const float*)P(w.hs), ha));
    if (last && out->hs)
      CK((int)hipMemcpyAsync(out->hs, P(w.hs), (size_t)BQ * 256 * 4, hipMemcpyDeviceToDevice, s));
    if (!last && out->aux_points)
      CK((int)hipMemcpyAsync(out->aux_points + aoff * 2, ref_buf(i + 1), (size_t)BQ * 2 * 4, hipMemcpyDeviceToDevice, s));
  }
  return 0;
}

// the stage bits in pipeline order: ENCODE stands for BACKBONE | TRANSFORMER; a mask must name neighbours
int rt_stage_mask(int stages) {
  const int all = SPE_STAGE_ENCODE | SPE_STAGE_DECODE | SPE_STAGE_BACKBONE | SPE_STAGE_TRANSFORMER;
  if (!stages || (stages & ~all)) return 0;
  if (stages & SPE_STAGE_ENCODE) stages = (stages & ~SPE_STAGE_ENCODE) | SPE_STAGE_BACKBONE | SPE_STAGE_TRANSFORMER;
  if ((stages & SPE_STAGE_BACKBONE) && (stages & SPE_STAGE_DECODE) && !(stages & SPE_STAGE_TRANSFORMER)) return 0;
  return stages;
}

int rt_forward_stages(spe_model* m, void* stream, const ImageSrc& images, bool u8, int B, void* workspace, int64_t ws_bytes,
                      const spe_rtdetr_outputs* out, int stages) {
  if (!m || !workspace || B <= 0) return fail(SPE_E_ARG, "bad argument");
  if (m->family != 1) return fail(SPE_E_ARG, "not an RT-DETR model");
  stages = rt_stage_mask(stages);
  if (!stages) return fail(SPE_E_ARG, "stages: a contiguous, non-empty set of SPE_STAGE_* bits");
  if ((stages & SPE_STAGE_BACKBONE) && !images.f32 && !images.u8) return fail(SPE_E_ARG, "null images");
  if ((stages & SPE_STAGE_DECODE) && (!out || !out->logits || !out->points)) return fail(SPE_E_ARG, "null outputs");
  if (u8 && images.ch != 1 && images.ch != 3) return fail(SPE_E_ARG, "u8 crops: 1 or 3 channels");
  if (!m->finalized) return fail(SPE_E_STATE, "model not finalized");
  const RtWs w = rt_plan(m, B);
  if ((int64_t)w.total > ws_bytes) return fail(SPE_E_WORKSPACE, "workspace too small");
  const RtModel& r = *m->rt;
  const RtFwd f{m, w, (char*)workspace, (hipStream_t)stream, B};
  if (stages & SPE_STAGE_BACKBONE)
    CK(r.ghost ? rt_backbone_ghostv2(m, f.s, images, B, f.ws, w)
       : r.mbv3 ? rt_backbone_mbv3(m, f.s, images, B, f.ws, w) : rt_backbone_presnet(m, f.s, images, B, f.ws, w));
  // (a stage's failing launch has recorded its own error)
  if (stages & SPE_STAGE_TRANSFORMER)
    if (const int rc = rt_encoder_stage(f)) return rc;
  if (stages & SPE_STAGE_DECODE)
    if (const int rc = rt_decoder_stage(f, out)) return rc;
  return 0;
}

}  // namespace

extern "C" {

int spe_rtdetr_forward(spe_model* m, void* stream, const float* images, int B, void* workspace, int64_t ws_bytes,
                       const spe_rtdetr_outputs* out) {
  return spe_rtdetr_forward_stages(m, stream, images, B, workspace, ws_bytes, out, SPE_STAGE_ENCODE | SPE_STAGE_DECODE);
}

int spe_rtdetr_forward_stages(spe_model* m, void* stream, const float* images, int B, void* workspace, int64_t ws_bytes,
                              const spe_rtdetr_outputs* out, int stages) {
  return rt_forward_stages(m, stream, ImageSrc{images, nullptr, 0}, false, B, workspace, ws_bytes, out, stages);
}

int spe_rtdetr_forward_stages_u8(spe_model* m, void* stream, const uint8_t* crops, int channels, int B, void* workspace,
                                 int64_t ws_bytes, const spe_rtdetr_outputs* out, int stages) {
  return rt_forward_stages(m, stream, ImageSrc{nullptr, crops, channels}, true, B, workspace, ws_bytes, out, stages);
}

}  // extern "C"
