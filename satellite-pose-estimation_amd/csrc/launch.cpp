// Launch helpers of the native runtime (launch.h), shared by the DETR (forward.cpp) and the UNC
// RT-DETR (rtdetr_*.cpp) launch sequences: every launch goes through run_gemm / run_attn /
// run_other, which bracket it with HIP events when the per-launch profiler is on
// (spe_model_profile_*, bench roofline), and through the fp32h3 activation-scale ledger.
#include "launch.h"

#include <cstdio>
#include <cstring>

namespace {

hipEvent_t next_event(spe_model* m) {
  Profiler& p = m->prof;
  if (p.next_event == p.pool.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    p.pool.push_back(e);
  }
  return p.pool[p.next_event++];
}

bool prof_match(const spe_model* m, const char* kind) {
  return m->prof.on && std::strncmp(kind, m->prof.filter.c_str(), m->prof.filter.size()) == 0;
}

// fp32h3 activation-scale ledger (one per forward call): every slot of a range the call zeroes must be
// raised by an earlier launch of the same call (GemmArgs::amax_c, the input pack, the cross-attention
// merge) before a launch reads it as its scale (amax_a and the like) -- a consumer without a producer
// would otherwise run at scale 1 in silence (h3_scale), losing precision or overflowing fp16.  Slots
// of ranges this call did not zero (a stage run by an earlier call) are not checked.
struct AmaxLedger {
  const float* base = nullptr;
  unsigned char state[SPE_AMAX_SLOTS] = {};     // 0 unchecked, 1 zeroed and awaiting a producer, 2 raised
  int index(const float* p) const {
    const long d = base && p ? (long)(p - base) : -1;
    return d >= 0 && d < SPE_AMAX_SLOTS ? (int)d : -1;
  }
  void zeroed(int first, int n) {
    for (int i = first; i < first + n; ++i) state[i] = 1;
  }
  void raised(const float* p) {
    const int i = index(p);
    if (i >= 0) state[i] = 2;
  }
  bool ok(const float* p) const {
    const int i = index(p);
    return i < 0 || state[i] != 1;
  }
};
thread_local AmaxLedger g_ledger_state;
thread_local AmaxLedger* g_ledger = nullptr;

}  // namespace

LedgerScope::LedgerScope(const float* base) {
  g_ledger_state = AmaxLedger{};
  g_ledger_state.base = base;
  g_ledger = base ? &g_ledger_state : nullptr;
}
LedgerScope::~LedgerScope() { g_ledger = nullptr; }
void LedgerScope::zeroed(int first, int n) { g_ledger_state.zeroed(first, n); }

int ledger_use(const float* in, const float* out, const char* kind) {
  if (!g_ledger) return 0;
  if (!g_ledger->ok(in)) {
    char b[160];
    snprintf(b, sizeof b, "fp32h3: %s reads activation-scale slot %d before any launch raised it", kind,
             g_ledger->index(in));
    return spe_fail(SPE_E_STATE, b);
  }
  g_ledger->raised(out);
  return 0;
}

int run_other(spe_model* m, const char* kind, double flops, double bytes, hipStream_t s, const std::function<int()>& fn) {
  if (!prof_match(m, kind)) return fn();
  ProfRecord r{kind, kind, flops, bytes, next_event(m), next_event(m)};
  if (!r.beg || !r.end) return (int)hipErrorOutOfMemory;
  (void)hipEventRecord(r.beg, s);
  int rc = fn();
  (void)hipEventRecord(r.end, s);
  m->prof.recs.push_back(r);
  return rc;
}

// fp32x3 models: split-bf16 MFMA.  fp32x6 models run the decoder's attention (self and cross,
// Q = 11 query rows: ~1 % of the model's flops) on the exact-f32 kernels: the per-stage study
//  found its split-bf16 scores to carry most of the mode's keypoint error
// (1.6e-4 -> 5.7e-5 on the bench weights at equal step time).
bool x3_for(const spe_model* m, const char* kind) {
  if (!m->x3) return false;
  if (m->x6 && std::strncmp(kind, "attn.dec", 8) == 0) return false;
  return true;
}

int run_gemm(spe_model* m, const char* kind, const GemmArgs& g, int mode, hipStream_t s) {
  if (const int rc = ledger_use(g.amax_a, g.amax_c, kind)) return rc;
  const double E = m->esz;
  const double a_elems = mode == GEMM_CONV ? (double)(g.M / (g.Ho * g.Wo)) * g.H * g.W * g.Cin : (double)g.M * g.K;
  const double r_rows = g.R ? (g.r_period > 0 ? (double)g.r_period : (double)g.M) : 0.0;
  const double bytes = (a_elems + (double)g.N * g.K + (double)g.M * g.N + r_rows * g.N) * E +
                       (mode == GEMM_LINEAR_ADD ? (double)g.prow * g.K * E : 0.0);
  int dt = !x3_for(m, kind) ? m->cfg.dtype : m->x6 ? (int)SPE_DTYPE_F32X6 : (int)SPE_DTYPE_F32X3;
  GemmArgs ga = g;
  if (dt == SPE_DTYPE_F32X6) {
    const auto it = m->w6.find(g.B);
    if (it != m->w6.end()) { ga.B6 = it->second.first; ga.b6_rows = it->second.second; }
    // fp32h3: the GEMMs whose A operand has a known max |A| (published by its producer, or a LayerNorm
    // / attention bound) take the scaled fp16 split (gemm.hip gemm_h3d / gemm_h3p); the rest stay on x6
    const auto ih = m->wh3.find(g.B);
    if (m->h3 && g.amax_a && ih != m->wh3.end()) {
      ga.H3 = ih->second.planes; ga.h3_rows = ih->second.rows; ga.h3_sinv = ih->second.sinv;
      dt = SPE_DTYPE_F32H3;
    }
  }
  return run_other(m, kind, 2.0 * g.M * g.N * g.K, bytes, s, [&] { return spe_launch_gemm(ga, dt, mode, s); });
}

int run_attn(spe_model* m, const char* kind, const AttnArgs& a, int dtype, hipStream_t s) {
  const double flops = 4.0 * a.B * a.H * (double)a.Tq * a.Tk * 32;
  const double bytes = (double)a.B * a.H * 32 * (2.0 * a.Tq + 2.0 * a.Tk) * m->esz;
  const int dt = (x3_for(m, kind) && dtype == SPE_DTYPE_F32) ? (int)SPE_DTYPE_F32X3 : dtype;
  if (const int rc = ledger_use(a.v_amax, nullptr, kind)) return rc;
  return run_other(m, kind, flops, bytes, s, [&] { return spe_launch_attention(a, dt, s); });
}

int run_layernorm(spe_model* m, const char* kind, const void* x, const float* g, const float* b, void* y, float* y32,
                  int M, int d, int dt, hipStream_t s) {
  const double bytes = (double)M * d * (m->esz + (y ? m->esz : 4));
  return run_other(m, kind, 0.0, bytes, s, [&] { return spe_launch_layernorm(x, g, b, y, y32, M, d, dt, s); });
}

GemmArgs linear_args(const Conv& c, const void* A, int lda, int M, void* C, int ldc) {
  GemmArgs g{};
  g.A = A; g.lda = lda;
  g.B = c.w; g.ldb = c.Kpad;
  g.M = M; g.N = c.N; g.K = c.K;
  g.bias = c.bias;
  g.C = C; g.ldc = ldc;
  return g;
}

GemmArgs conv_args(const Conv& c, const void* X, int B, int H, int W, void* Y, int ldc) {
  GemmArgs g{};
  g.A = X;
  g.H = H; g.W = W; g.Cin = c.Cin; g.KH = c.KH; g.KW = c.KW; g.stride = c.stride; g.pad = c.pad;
  g.Ho = (H + 2 * c.pad - c.KH) / c.stride + 1;
  g.Wo = (W + 2 * c.pad - c.KW) / c.stride + 1;
  g.B = c.w; g.ldb = c.Kpad;
  g.M = B * g.Ho * g.Wo; g.N = c.N; g.K = c.K;
  g.bias = c.bias;
  g.C = Y; g.ldc = ldc;
  return g;
}

// `(x + pos) . W^T`: fp32 / fp32x3 models add pos to the A operand as the reference does; bf16
// and fp32x6 models add the precomputed pos . W^T as a row-periodic residual (see gemm2.hip).
int add_pos(const spe_model* m, GemmArgs& g, const void* pos, int ldp, int period, const void* posw, int ldw) {
  if ((m->esz == 2 || m->x6) && posw) {
    g.R = posw; g.ldr = ldw; g.r_period = period;
    return GEMM_LINEAR;
  }
  g.P = pos; g.ldp = ldp; g.prow = period;
  return GEMM_LINEAR_ADD;
}

// what both forms of the fused bf16 FFN (ffn.hip) take: M rows of x through l1 / l2 into y, LayerNorm g / b
static FfnArgs ffn_args(const Conv& l1, const Conv& l2, const float* g, const float* b, const void* x, void* y, int M,
                        const void* pos, void* ypos, int period, float* partial, const void* w2_chunked) {
  FfnArgs a{};
  a.pos = pos; a.ypos = ypos; a.pos_period = period;
  a.splits = partial ? spe_ffn_splits(M, l1.N) : 1;
  a.partial = a.splits > 1 ? partial : nullptr;
  a.x = x; a.ldx = l1.K;
  a.w1 = l1.w; a.ld1 = l1.Kpad; a.b1 = l1.bias;
  a.w2 = w2_chunked ? w2_chunked : l2.w; a.ld2 = l2.Kpad; a.b2 = l2.bias;
  a.w2_chunked = w2_chunked != nullptr;        // W2 chunk-packed at finalize (ffn.hip)
  a.gamma = g; a.beta = b;
  a.y = y; a.ldy = l1.K;
  a.M = M; a.D = l1.K; a.F = l1.N;
  return a;
}

// Fused linear1 -> ReLU -> linear2 -> +residual -> LayerNorm over x (in place), bf16 models.
int run_ffn(spe_model* m, const char* kind, const Conv& l1, const Conv& l2, const float* g, const float* b,
            void* x, int M, hipStream_t s, const void* pos, void* ypos, int period, float* partial,
            const void* w2_chunked) {
  const FfnArgs a = ffn_args(l1, l2, g, b, x, x, M, pos, ypos, period, partial, w2_chunked);
  const double flops = 4.0 * M * (double)l1.K * l1.N;
  const double bytes = 2.0 * M * l1.K * m->esz + 2.0 * (double)l1.K * l1.N * m->esz;
  return run_other(m, kind, flops, bytes, s, [&] { return spe_launch_ffn_ln(a, s); });
}

// The pre-norm form (ffn.hip spe_launch_ffn_pre): y = x + W2 relu(W1 LN(x; g, b) + b1) + b2 and y2 = LN(y; g2, b2n)
// beside it (y2 null: not stored), ypos = y2 + pos.  x and y may alias.
int run_ffn_pre(spe_model* m, const char* kind, const Conv& l1, const Conv& l2, const float* g, const float* b,
                const void* x, void* y, const float* g2, const float* b2n, void* y2, int M, hipStream_t s, const void* pos,
                void* ypos, int period, float* partial, const void* w2_chunked) {
  FfnArgs a = ffn_args(l1, l2, g, b, x, y, M, pos, ypos, period, partial, w2_chunked);
  a.gamma2 = g2; a.beta2 = b2n; a.y2 = y2;
  const double flops = 4.0 * M * (double)l1.K * l1.N;
  const double bytes = (2.0 + (y2 ? 1.0 : 0.0) + (ypos ? 1.0 : 0.0)) * M * l1.K * m->esz + 2.0 * (double)l1.K * l1.N * m->esz;
  return run_other(m, kind, flops, bytes, s, [&] { return spe_launch_ffn_pre(a, s); });
}

extern "C" {

int spe_model_profile_begin(spe_model* m, const char* kind_prefix) {
  if (!m) return spe_fail(SPE_E_ARG, "null model");
  m->prof.on = true;
  m->prof.filter = kind_prefix ? kind_prefix : "";
  m->prof.recs.clear();
  m->prof.next_event = 0;
  return 0;
}

int spe_model_profile_end(spe_model* m) {
  if (!m) return spe_fail(SPE_E_ARG, "null model");
  m->prof.on = false;
  for (auto& r : m->prof.recs) {
    hipError_t e = hipEventSynchronize(r.end);
    if (e != hipSuccess) return spe_fail((int)e, "profile event sync failed");
  }
  return (int)m->prof.recs.size();
}

int spe_model_profile_get(const spe_model* m, int i, char* kind, int kind_len, double* ms, double* flops,
                          double* bytes) {
  if (!m || i < 0 || i >= (int)m->prof.recs.size()) return spe_fail(SPE_E_ARG, "bad profile record index");
  const ProfRecord& r = m->prof.recs[i];
  if (kind && kind_len > 0) {
    std::strncpy(kind, r.kind.c_str(), kind_len - 1);
    kind[kind_len - 1] = 0;
  }
  float t = 0.f;
  hipError_t e = hipEventElapsedTime(&t, r.beg, r.end);
  if (e != hipSuccess) return spe_fail((int)e, "hipEventElapsedTime failed");
  if (ms) *ms = t;
  if (flops) *flops = r.flops;
  if (bytes) *bytes = r.bytes;
  return 0;
}

}  // extern "C"
