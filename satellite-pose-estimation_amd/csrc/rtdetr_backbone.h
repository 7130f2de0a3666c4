// The RT-DETR runtime's backbone interface: rtdetr_model.cpp (parameter-space tail, workspace plan, HybridEncoder,
// decoder, C entry points) reaches a backbone family only through its RtBackbone row.  A new backbone is one
// rtdetr_<family>.cpp defining its row, one entry in rt_backbone_for's table and one word in the Makefile.
#pragma once
#include "launch.h"
#include "model_state.h"
#include "registry.h"

// parameter keys and shapes in the reference's state_dict order
struct RtSpec {
  std::vector<std::pair<std::string, std::vector<int64_t>>> keys;
  void add(const std::string& k, std::vector<int64_t> sh) { keys.emplace_back(k, std::move(sh)); }
  void bn(const std::string& p, int64_t ch) {
    for (const char* n : {"weight", "bias", "running_mean", "running_var"}) add(p + "." + n, {ch});
  }
  void cnl(const std::string& p, int64_t cin, int64_t cout, int64_t k) {   // ConvNormLayer
    add(p + ".conv.weight", {cout, cin, k, k});
    bn(p + ".norm", cout);
  }
  void lin(const std::string& p, int64_t o, int64_t i) { add(p + ".weight", {o, i}); add(p + ".bias", {o}); }
};

// largest tiles x channels product of an SE block's pool partials (block 11: 4 tiles x 672 at 256 input)
constexpr size_t MB_POOL_MAX = 4096;

// ---- workspace plan (byte offsets)
struct RtWs {
  size_t x0, bufA, bufB, t1, t2, sc, f0, f1, f2;
  size_t cat0, cat1, catp0, catp1, aqk, avt, aao, atmp, affn, aout;
  size_t x1, x2, y, inner1, p3, n4, n5;
  size_t mbpool, mbscale;      // se_scratch backbones: dwconv pool partials [B][MB_POOL_MAX], SE scales [B][960]
  size_t mem, omem, elog, value;
  size_t topk, tgt, slog, sanc, refs, qh, qpos, hh1, hh2, dqk, dvt, dao, dtmp, t1d, t2d, soaw, dcr, dffn, hs, lgt;
  size_t total;
};

struct RtBackbone {
  bool (*selects)(const spe_rtdetr_config&);              // reads cfg.depth
  const char* (*refuses)(const spe_rtdetr_config&);       // nullptr, or spe_rtdetr_create's SPE_E_ARG message
  void (*channels)(const spe_rtdetr_config&, int fch[3]); // f0 / f1 / f2 widths
  void (*spec)(const spe_rtdetr_config&, RtSpec&);        // the "backbone.*" keys, in registration order
  int (*build)(spe_model*);                               // fold + pack + upload (two-pass finalize)
  // images -> f0 / f1 / f2 (NHWC, strides 8 / 16 / 32) where the hybrid encoder reads them
  int (*run)(spe_model*, hipStream_t, const ImageSrc&, int B, char* ws, const RtWs&);
  bool se_scratch;                                        // needs mbpool / mbscale in the plan
};
// each family's row (a function-local static: host data only), in rtdetr_presnet.cpp, rtdetr_mbv3.cpp, rtdetr_ghostv2.cpp
const RtBackbone* rt_bb_presnet();
const RtBackbone* rt_bb_mbv3();
const RtBackbone* rt_bb_ghostv2();
inline const RtBackbone* rt_backbone_for(const spe_rtdetr_config& c) {   // nullptr: no family takes this depth
  for (const RtBackbone* b : {rt_bb_presnet(), rt_bb_mbv3(), rt_bb_ghostv2()})
    if (b->selects(c)) return b;
  return nullptr;
}

// bytes a backbone's first launch reads per input pixel: the fp32 batch's three channels or the crop's 1 / 3
inline double image_px_bytes(const ImageSrc& img) { return img.u8 ? (double)img.ch : 12.0; }

// ---- packing and launches the light backbones share (defined in rtdetr_mbv3.cpp, beside mbv3.hip's first user)
Conv mb_conv(spe_model* m, const std::string& wkey, const std::string& bn, const std::string& biaskey, int stride,
             int pad, bool pool2 = false);
MbDw mb_dw(spe_model* m, const std::string& wkey, const std::string& bn, int stride);
struct MbRun {               // one backbone call
  spe_model* m;
  hipStream_t s;
  int B;
};
// "conv.pw.mb": 1x1 conv (or an implicit GEMM) over an NHWC map of edge Hin; R (nullable) is added before act,
// scale (nullable) is the SE gate on A
int mb_run_pw(const MbRun& x, const Conv& cv, const void* in, int Hin, void* outp, int act, const void* R, const float* scale);
// "conv.dw": depthwise conv; pool (nullable) receives the SE pool partials
int mb_run_dw(const MbRun& x, const MbDw& d, const void* in, int Hin, void* outp, int act, float* pool);
// "rt.se": pool partials of a C-channel map of edge Ho -> scale [B][C]
int mb_run_se(const MbRun& x, const MbSe& g, const float* pool, int tiles, int Ho, int C, float* scale);
