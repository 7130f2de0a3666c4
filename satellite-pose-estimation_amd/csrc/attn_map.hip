// Head-averaged attention probabilities (the `need_weights=True` output of nn.MultiheadAttention
// that the flash kernels never form) for gfx950: the diagnostic tap behind spe_forward_attention.
//
//   out[b][i][j] = (1/H) sum_h softmax_j(scale . q_h[b][i] . k_h[b][j])        fp32 [B][Tq][Tk], H = 8
//
// The reference's visualize_features.py reads it from transformer.encoder.layers[-1].self_attn
// (Tq = Tk = tokens) and transformer.decoder.layers[-2].multihead_attn (Tq = queries, Tk = tokens).
//
// One wave owns 16 query rows of one image; a work-group is 4 such waves (64 rows) that walk the
// keys together so K tiles are shared through the vector L1.  No LDS, no barriers, no atomics.
// Scores are computed transposed (S^T = K . Q^T, v_mfma_f32_16x16x32_{bf16,f16} or the exact-f32
// v_mfma_f32_16x16x4_f32): the query sits on the lane (l & 15), so a row's max and sum are per-lane
// scalars combined once across the four lane groups (l >> 4).  The A rows of the four MFMAs of a 64-key
// tile are assigned keys 16 (a >> 2) + 4 t + (a & 3) (a = A row, t = MFMA), which leaves lane group g
// holding the 16 CONSECUTIVE keys 16 g .. 16 g + 15 of its query row: four 16-byte stores per lane, a
// 256-byte run per row and tile.
//
// Two passes over the keys (the row softmax needs the whole row before anything can be written, and a
// [16][Tk] fp32 row tile does not fit LDS at Tk = 2704 .. 6400):
//   1. per head: the row max m_h and sum l_h = sum_j exp(s - m_h), one sweep with a running max
//   2. per 64-key tile: the scores of all 8 heads again, p = exp(s - m_h) / l_h summed over the heads
//      in registers, times 1/8, each output element written once with plain vector stores.
// Scores, max, sum and the head average are fp32; exp is the full-precision expf / exp2f.
//
// Operand forms (AttnMapArgs): head_dim 32 with per-head q and k (the encoder's qkv buffer, the
// fp32 decoder's dqc / ck), or head_dim 256 with one k shared by the heads and q pre-scaled into the
// exp2 domain (the bf16 decoder's folded cross-attention, xattn.hip: q' = (tgt + query_pos) . Wqk^T against
// memory + pos).  Rows past Tq / keys past Tk are clamped for the loads and masked / not stored.
#include "spe_common.h"
#include <type_traits>
#include "spe_kernels.h"

namespace {

constexpr int NT = 256;                // 4 waves
constexpr int ROWS = 16;               // query rows per wave
constexpr int KT = 64;                 // keys per tile
constexpr int H = 8;
constexpr float NEG_BIG = -1.0e30f;    // finite "minus infinity"

struct f16_tag {};                     // element tags: bf16 / f16_tag (16-bit), float

template <typename T> struct Elem { static constexpr int ES = 2; };
template <> struct Elem<float> { static constexpr int ES = 4; };

// one 16x16 block of S^T over NCH 64-byte K-steps: a = K fragment (A), b = Q fragment (B)
template <typename T, int NCH>
SPE_DEV f32x4 block_mma(const u32x4* a, const u32x4* b) {
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < NCH; ++kk) {
    if constexpr (sizeof(T) == 4) {
      const f32x4 fa = __builtin_bit_cast(f32x4, a[kk]), fb = __builtin_bit_cast(f32x4, b[kk]);
#pragma unroll
      for (int s = 0; s < 4; ++s) c = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[s], fb[s], c, 0, 0, 0);
    } else if constexpr (std::is_same_v<T, f16_tag>) {
      c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a[kk]), __builtin_bit_cast(f16x8, b[kk]), c, 0,
                                                 0, 0);
    } else {
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[kk]), __builtin_bit_cast(bf16x8, b[kk]), c,
                                                  0, 0, 0);
    }
  }
  return c;
}

// T: element tag; D: head_dim (32 or 256); BASE2: scores already in the exp2 domain (scale folded into q)
template <typename T, int D, bool BASE2>
__global__ __launch_bounds__(NT) void attn_map_kernel(AttnMapArgs a) {
  constexpr int ES = Elem<T>::ES;
  constexpr int NCH = D * ES / 64;          // 16-byte chunks per lane and row: chunk kk at byte 64 kk + 16 g
  constexpr bool HOLDQ = H * NCH <= 16;     // every head's Q fragment stays in registers (head_dim 32)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int b = blockIdx.y;
  const int i0 = (blockIdx.x * (NT / 64) + wave) * ROWS;
  if (i0 >= a.Tq) return;                   // wave-uniform; the kernel has no barrier
  const int i = i0 + r;                     // this lane's query row
  const int il = i < a.Tq ? i : a.Tq - 1;   // clamped for the loads
  const char* qrow = (const char*)a.q + ((size_t)b * a.q_sb + (size_t)il * a.ldq) * ES + g * 16;
  const char* kimg = (const char*)a.k + (size_t)b * a.k_sb * ES + g * 16;
  // this lane's A row r of MFMA t holds key 16 (r >> 2) + 4 t + (r & 3) of the tile
  const int kl = 16 * (r >> 2) + (r & 3);
  const int ntiles = (a.Tk + KT - 1) / KT;

  u32x4 qf[HOLDQ ? H : 1][NCH];
  auto load_q = [&](int h, u32x4* dst) {
    const char* p = qrow + (size_t)h * a.q_sh * ES;
#pragma unroll
    for (int kk = 0; kk < NCH; ++kk) dst[kk] = ld16(p + kk * 64);
  };
  if constexpr (HOLDQ) {
#pragma unroll
    for (int h = 0; h < H; ++h) load_q(h, qf[h]);
  }

  // the scores of this lane's query against keys j0 + 16 g + 4 t + e (s[4 t + e]), scaled and masked
  auto scores = [&](int h, int j0, const u32x4* q, float* s) {
    const char* kh = kimg + (size_t)h * a.k_sh * ES;
    u32x4 kf[4][NCH];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      int key = j0 + kl + 4 * t;
      key = key < a.Tk ? key : a.Tk - 1;
      const char* p = kh + (size_t)key * a.ldk * ES;
#pragma unroll
      for (int kk = 0; kk < NCH; ++kk) kf[t][kk] = ld16(p + kk * 64);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 c = block_mma<T, NCH>(kf[t], q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = j0 + 16 * g + 4 * t + e;
        const float v = BASE2 ? c[e] : c[e] * a.scale;
        s[4 * t + e] = j < a.Tk ? v : NEG_BIG;
      }
    }
  };
  auto ex = [](float x) { return BASE2 ? exp2f(x) : expf(x); };

  // ---- pass 1: row max and sum of every head
  float mh[H], lh[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    u32x4 qtmp[NCH];
    const u32x4* q;
    if constexpr (HOLDQ) {
      q = qf[h];
    } else {
      load_q(h, qtmp);
      q = qtmp;
    }
    float m = NEG_BIG, l = 0.f;
    for (int kt = 0; kt < ntiles; ++kt) {
      float s[16];
      scores(h, kt * KT, q, s);
      float tm = s[0];
#pragma unroll
      for (int e = 1; e < 16; ++e) tm = fmaxf(tm, s[e]);
      tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
      tm = fmaxf(tm, __shfl_xor(tm, 32, 64));       // the tile's row max, the same on the row's four lanes
      const float mn = fmaxf(m, tm);                // (key 0 of the first tile is always valid: mn is finite)
      float ps = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) ps += ex(s[e] - mn);
      l = l * ex(m - mn) + ps;
      m = mn;
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    mh[h] = m;
    lh[h] = l;
  }

  // ---- pass 2: normalise, average the heads, write each element once
  float* orow = a.out + ((size_t)b * a.Tq + il) * a.Tk;
  const bool live = i < a.Tq;
  const bool vec = (a.Tk & 3) == 0;                 // every row 16-byte aligned (the base pointer is checked)
  for (int kt = 0; kt < ntiles; ++kt) {
    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      u32x4 qtmp[NCH];
      const u32x4* q;
      if constexpr (HOLDQ) {
        q = qf[h];
      } else {
        load_q(h, qtmp);
        q = qtmp;
      }
      float s[16];
      scores(h, kt * KT, q, s);
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] += ex(s[e] - mh[h]) / lh[h];
    }
    // (rows past Tq only skip the stores: no divergent control flow around the MFMAs)
    const int j = kt * KT + 16 * g;
    if (vec) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (live && j + 4 * t < a.Tk)               // Tk % 4 == 0: a quad is whole or absent
          *reinterpret_cast<f32x4*>(orow + j + 4 * t) = f32x4{acc[4 * t] * 0.125f, acc[4 * t + 1] * 0.125f,
                                                               acc[4 * t + 2] * 0.125f, acc[4 * t + 3] * 0.125f};
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (live && j + e < a.Tk) orow[j + e] = acc[e] * 0.125f;
    }
  }
}

template <typename T, int D, bool BASE2>
int launch(const AttnMapArgs& a, hipStream_t s) {
  const dim3 grid((a.Tq + 4 * ROWS - 1) / (4 * ROWS), a.B);
  hipLaunchKernelGGL((attn_map_kernel<T, D, BASE2>), grid, dim3(NT), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace

int spe_launch_attn_map(const AttnMapArgs& a, int dtype, hipStream_t s) {
  const int es = dtype == SPE_DTYPE_F32 ? 4 : 2;
  if (dtype != SPE_DTYPE_F32 && dtype != SPE_DTYPE_BF16 && dtype != SPE_DTYPE_F16) return -1;
  if (!a.q || !a.k || !a.out || a.B <= 0 || a.B > 65535 || a.H != H || a.Tq <= 0 || a.Tk <= 0) return -1;
  if (a.head_dim != 32 && !(a.head_dim == 256 && a.base2 && dtype == SPE_DTYPE_BF16)) return -1;
  if (a.base2 && a.head_dim != 256) return -1;
  // every fragment load is 16 bytes: rows, heads and images start on 16-byte boundaries
  auto al = [&](long long elems) { return (elems * es) % 16 == 0; };
  if (!al(a.ldq) || !al(a.ldk) || !al(a.q_sb) || !al(a.k_sb) || !al(a.q_sh) || !al(a.k_sh)) return -1;
  if (a.ldq < a.head_dim || a.ldk < a.head_dim) return -1;
  if (((uintptr_t)a.q | (uintptr_t)a.k) & 15) return -1;
  if ((uintptr_t)a.out & ((a.Tk & 3) == 0 ? 15 : 3)) return -1;   // the 16-byte stores (Tk % 4 == 0)
  if (a.head_dim == 256) return launch<bf16, 256, true>(a, s);
  if (dtype == SPE_DTYPE_F32) return launch<float, 32, false>(a, s);
  if (dtype == SPE_DTYPE_F16) return launch<f16_tag, 32, false>(a, s);
  return launch<bf16, 32, false>(a, s);
}
