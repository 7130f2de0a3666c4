// Launch helpers of the native runtime (launch.cpp), shared by the DETR (forward.cpp) and the UNC
// RT-DETR (rtdetr_*.cpp) launch sequences: every launch goes through run_gemm / run_attn /
// run_other, which bracket it with HIP events when the per-launch profiler is on
// (spe_model_profile_*, bench roofline).
#pragma once
#include <cstdio>
#include <functional>

#include "model_state.h"

// return from the calling entry point with the failing call recorded as the last error
#define CK(x)                                                                         \
  do {                                                                                \
    int _r = (x);                                                                     \
    if (_r != 0) {                                                                    \
      char _b[256];                                                                   \
      snprintf(_b, sizeof _b, "%s failed (%d) at %s:%d", #x, _r, __FILE__, __LINE__);  \
      return spe_fail(_r < 0 ? SPE_E_LAUNCH : _r, _b);                                \
    }                                                                                 \
  } while (0)

// The fp32h3 activation-scale ledger of one forward call, live while the scope is: `base` is the call's
// slot array in the workspace (null: no ledger, every check passes).
struct LedgerScope {
  explicit LedgerScope(const float* base);
  ~LedgerScope();
  LedgerScope(const LedgerScope&) = delete;
  void zeroed(int first, int n);   // the call zeroed slots [first, first + n): each now awaits a producer
};
// a launch reading `in` and raising `out`: SPE_E_STATE if `in` has no producer yet
int ledger_use(const float* in, const float* out, const char* kind);

int run_other(spe_model* m, const char* kind, double flops, double bytes, hipStream_t s, const std::function<int()>& fn);
int run_gemm(spe_model* m, const char* kind, const GemmArgs& g, int mode, hipStream_t s);
int run_attn(spe_model* m, const char* kind, const AttnArgs& a, int dtype, hipStream_t s);
// LayerNorm of M rows of d: x -> y (the model's dtype) and / or y32 (fp32)
int run_layernorm(spe_model* m, const char* kind, const void* x, const float* g, const float* b, void* y, float* y32,
                  int M, int d, int dt, hipStream_t s);
bool x3_for(const spe_model* m, const char* kind);
GemmArgs linear_args(const Conv& c, const void* A, int lda, int M, void* C, int ldc);
GemmArgs conv_args(const Conv& c, const void* X, int B, int H, int W, void* Y, int ldc);
int add_pos(const spe_model* m, GemmArgs& g, const void* pos, int ldp, int period, const void* posw, int ldw);
int run_ffn(spe_model* m, const char* kind, const Conv& l1, const Conv& l2, const float* g, const float* b, void* x,
            int M, hipStream_t s, const void* pos = nullptr, void* ypos = nullptr, int period = 0,
            float* partial = nullptr, const void* w2_chunked = nullptr);
// the pre-norm form: y = x + FFN(LN(x; g, b)), y2 = LN(y; g2, b2n) beside it (null: not stored), ypos = y2 + pos
int run_ffn_pre(spe_model* m, const char* kind, const Conv& l1, const Conv& l2, const float* g, const float* b,
                const void* x, void* y, const float* g2, const float* b2n, void* y2, int M, hipStream_t s,
                const void* pos = nullptr, void* ypos = nullptr, int period = 0, float* partial = nullptr,
                const void* w2_chunked = nullptr);
