// PResNet-vd backbone of the RT-DETR runtime (UNC/nn/backbone/presnet.py:156-265), depths 18 (BasicBlock) and 50
// (BottleNeck): parameter keys, packing and the launch sequence behind the RtBackbone row rt_bb_presnet.  The
// variant-d shortcut AvgPool2d(2, 2, ceil_mode) + 1x1 conv is folded into one 2x2 stride-2 conv with w/4 per tap
// (exact for the even feature sizes of inputs that are multiples of 32).
#include "rtdetr_backbone.h"

namespace {

const int RESNET_CFG18[4] = {2, 2, 2, 2}, RESNET_CFG50[4] = {3, 4, 6, 3};

bool bottleneck(const spe_rtdetr_config& c) { return c.depth >= 50; }

void presnet_spec(const spe_rtdetr_config& c, RtSpec& s) {
  const bool bott = bottleneck(c);
  const int64_t exp = bott ? 4 : 1;
  s.cnl("backbone.conv1.conv1_1", 3, 32, 3);
  s.cnl("backbone.conv1.conv1_2", 32, 32, 3);
  s.cnl("backbone.conv1.conv1_3", 32, 64, 3);
  const int* nb = bott ? RESNET_CFG50 : RESNET_CFG18;
  const int64_t widths[4] = {64, 128, 256, 512};
  int64_t cin = 64;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < nb[i]; ++j) {
      const std::string p = "backbone.res_layers." + std::to_string(i) + ".blocks." + std::to_string(j);
      const int64_t co = widths[i];
      const bool s2 = j == 0 && i > 0;
      auto shortcut = [&] { if (j == 0) s.cnl(s2 ? p + ".short.conv" : p + ".short", cin, co * exp, 1); };
      if (bott) {
        s.cnl(p + ".branch2a", cin, co, 1);
        s.cnl(p + ".branch2b", co, co, 3);
        s.cnl(p + ".branch2c", co, co * exp, 1);
        shortcut();
      } else {                       // BasicBlock registers `short` before its branches
        shortcut();
        s.cnl(p + ".branch2a", cin, co, 3);
        s.cnl(p + ".branch2b", co, co, 3);
      }
      cin = co * exp;
    }
}

int presnet_build(spe_model* m) {
  RtPresnet& r = m->rt->pr;
  r.blocks.clear();
  const std::string bb = "backbone.conv1.conv1_";
  r.stem[0] = make_conv(m, bb + "1.conv.weight", bb + "1.norm", "", 8, 2, 1);
  r.stem[1] = make_conv(m, bb + "2.conv.weight", bb + "2.norm", "", 0, 1, 1);
  r.stem[2] = make_conv(m, bb + "3.conv.weight", bb + "3.norm", "", 0, 1, 1);
  const bool bott = bottleneck(m->rt->cfg);
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
  return 0;
}

int rt_backbone_presnet(spe_model* m, hipStream_t s, const ImageSrc& images, int B, char* ws, const RtWs& w) {
  const RtPresnet& r = m->rt->pr;
  const auto& c = m->rt->cfg;
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

}  // namespace

const RtBackbone* rt_bb_presnet() {
  static const RtBackbone bb = {
      [](const spe_rtdetr_config& c) { return c.depth == 18 || c.depth == 50; },
      [](const spe_rtdetr_config&) -> const char* { return nullptr; },
      [](const spe_rtdetr_config& c, int fch[3]) {
        for (int l = 0; l < 3; ++l) fch[l] = (128 << l) * (bottleneck(c) ? 4 : 1);
      },
      presnet_spec, presnet_build, rt_backbone_presnet, false};
  return &bb;
}

