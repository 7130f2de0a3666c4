// MobileNetV3_Large backbone kernels of the UNC RT-DETR model (UNC/nn/backbone/mobilenetv3.py:28-225),
// gfx950, NHWC, storage T = bf16 (fp32 accumulation) or float (exact-f32 MFMA):
//
//   mb_stem      conv1 3x3/s2 3 -> 16 + folded BN + Hardswish, read straight from the fp32 NCHW batch, or
//                (mb_stem_u8) from the 8-bit crops it is normalised from, tiled through LDS
//   mb_dwconv    depthwise k x k (k 3 / 5, stride 1 / 2, pad k/2) + folded BN + none / ReLU / Hardswish;
//                an 8 x 8 output tile x a group of 16-byte channel vectors per work-group, the input
//                patch with its halo staged once in LDS; optionally the per-(image, tile, channel) sums
//                of the stored outputs, reduced in a fixed order (no floating-point atomics): the SE
//                gate's pool without a second pass over the expanded tensor
//   mb_se_gate   pooled mean -> fc1 + folded BN + ReLU -> fc2 (+ bias, GhostNetV2) -> Hardsigmoid -> fp32 [B][C]
//                scales, one work-group per image, one launch per block
//   mb_gemm      C = act((A * scale) . W^T + bias + R): the 1x1 convolutions (expand, project, skip) and,
//                through the implicit-GEMM A loader, Conv1 / Conv2; the SE scale is applied to the A
//                operand while it is staged, the residual is added BEFORE the activation
//                (Block.forward: act3(bn3(conv3(.)) + skip)); 64 x 64 tiles, MFMA 16x16x32 bf16 /
//                16x16x4 f32, register-prefetched K stages of 128 bytes a row
#include <hip/hip_runtime.h>

#include "spe_common.h"
#include "spe_kernels.h"
#include "stem_u8.h"

namespace {

SPE_DEV float mb_act(float v, int act) {
  if (act == MB_ACT_RELU) return fmaxf(v, 0.f);
  if (act == MB_ACT_HSWISH) return v * fminf(fmaxf(v + 3.f, 0.f), 6.f) / 6.f;
  return v;
}

// ---------------------------------------------------------------- stem
// thread = one output pixel, 16 channels; weights [27][16] (k = (ci*3 + kh)*3 + kw) + bias in LDS
template <typename T>
__global__ __launch_bounds__(256) void mb_stem_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                      const float* __restrict__ bias, T* __restrict__ out, int B, int S) {
  __shared__ float wl[27 * 16 + 16];
  for (int i = threadIdx.x; i < 27 * 16 + 16; i += 256) wl[i] = i < 432 ? w[i] : bias[i - 432];
  __syncthreads();
  const int So = S >> 1;
  const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= (size_t)B * So * So) return;
  const int ox = (int)(pix % So), oy = (int)((pix / So) % So), b = (int)(pix / ((size_t)So * So));
  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = wl[432 + c];
  for (int ci = 0; ci < 3; ++ci)
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int iy = 2 * oy - 1 + kh;
      if (iy < 0 || iy >= S) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int ix = 2 * ox - 1 + kw;
        if (ix < 0 || ix >= S) continue;
        const float x = img[(((size_t)b * 3 + ci) * S + iy) * S + ix];
        const float* wk = &wl[((ci * 3 + kh) * 3 + kw) * 16];
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[c] = fmaf(x, wk[c], acc[c]);
      }
    }
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = mb_act(acc[c], MB_ACT_HSWISH);
  constexpr int CE = Chunk<T>::CE;
  T* o = out + pix * 16;
#pragma unroll
  for (int c = 0; c < 16; c += CE) st16(o + c, pack16<T>(acc + c));
}

// the same stem from the 8-bit crops [B][S][S][CH]: a 16 x 16 output tile a work-group, the patch staged and
// normalised once in LDS (stem_u8.h); bit-identical to mb_stem_kernel on the batch normalised that way
template <typename T, int CH>
__global__ __launch_bounds__(256) void mb_stem_u8_kernel(const uint8_t* __restrict__ crops, const float* __restrict__ w,
                                                         const float* __restrict__ bias, T* __restrict__ out, int S) {
  __shared__ float wl[27 * 16 + 16];
  __shared__ StemU8Lds lds;
  for (int i = threadIdx.x; i < 27 * 16 + 16; i += 256) wl[i] = i < 432 ? w[i] : bias[i - 432];
  const int So = S >> 1, tiles_x = So / SU_T;
  const int ty0 = (blockIdx.x / tiles_x) * SU_T, tx0 = (blockIdx.x % tiles_x) * SU_T, b = blockIdx.y;
  stem_u8_stage<CH>(crops, S, b, ty0, tx0, lds);          // (its barriers cover wl)
  const int ox = threadIdx.x & (SU_T - 1), oy = threadIdx.x / SU_T, gy = ty0 + oy, gx = tx0 + ox;
  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = wl[432 + c];
  stem_u8_accumulate(lds.x, wl, S, gy, gx, oy, ox, acc);
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = mb_act(acc[c], MB_ACT_HSWISH);
  constexpr int CE = Chunk<T>::CE;
  T* o = out + (((size_t)b * So + gy) * So + gx) * 16;
#pragma unroll
  for (int c = 0; c < 16; c += CE) st16(o + c, pack16<T>(acc + c));
}

// ---------------------------------------------------------------- depthwise
constexpr int DW_T = 8;                       // output tile edge
constexpr int DW_PMAX = (DW_T - 1) * 2 + 5;   // patch edge at stride 2, k 5
constexpr int DW_CGMAX = 8;                   // 16-byte channel vectors per work-group

template <typename T>
__global__ __launch_bounds__(256) void mb_dwconv_kernel(MbDwArgs a) {
  constexpr int CE = Chunk<T>::CE;
  __shared__ u32x4 patch[DW_PMAX * DW_PMAX * DW_CGMAX];
  __shared__ float wl[25 * DW_CGMAX * 8];
  const int CG = a.cg, CGC = CG * CE, nvec = a.C / CE;
  const int tiles_x = (a.Wo + DW_T - 1) / DW_T;
  const int tile = blockIdx.x, ty0 = (tile / tiles_x) * DW_T, tx0 = (tile % tiles_x) * DW_T;
  const int gv0 = blockIdx.y * CG, b = blockIdx.z;
  const int k = a.k, s = a.stride, pad = k >> 1;
  const int PW = (DW_T - 1) * s + k;
  const T* in = (const T*)a.in + (size_t)b * a.H * a.W * a.C;
  for (int i = threadIdx.x; i < PW * PW * CG; i += 256) {
    const int cv = i % CG, p = i / CG, py = p / PW, px = p - py * PW;
    const int iy = ty0 * s - pad + py, ix = tx0 * s - pad + px;
    u32x4 v{0u, 0u, 0u, 0u};
    if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W && gv0 + cv < nvec)
      v = ld16(in + ((size_t)iy * a.W + ix) * a.C + (size_t)(gv0 + cv) * CE);
    patch[i] = v;
  }
  for (int i = threadIdx.x; i < k * k * CGC; i += 256) {
    const int tap = i / CGC, c = i - tap * CGC, ch = gv0 * CE + c;
    wl[i] = ch < a.C ? a.w[(size_t)tap * a.C + ch] : 0.f;
  }
  __syncthreads();
  const int cv = threadIdx.x % CG, slot = threadIdx.x / CG, nslots = 256 / CG;
  const bool cvalid = gv0 + cv < nvec;
  float bs[CE], psum[CE];
#pragma unroll
  for (int e = 0; e < CE; ++e) {
    bs[e] = cvalid ? a.bias[(gv0 + cv) * CE + e] : 0.f;
    psum[e] = 0.f;
  }
  for (int p = slot; p < DW_T * DW_T; p += nslots) {
    const int oy = p / DW_T, ox = p % DW_T, gy = ty0 + oy, gx = tx0 + ox;
    if (!cvalid || gy >= a.Ho || gx >= a.Wo) continue;
    float acc[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) acc[e] = bs[e];
    for (int kh = 0; kh < k; ++kh)
      for (int kw = 0; kw < k; ++kw) {
        float x[CE];
        unpack16<T>(patch[((oy * s + kh) * PW + ox * s + kw) * CG + cv], x);
        const float* wk = &wl[(kh * k + kw) * CGC + cv * CE];
#pragma unroll
        for (int e = 0; e < CE; ++e) acc[e] = fmaf(x[e], wk[e], acc[e]);
      }
#pragma unroll
    for (int e = 0; e < CE; ++e) acc[e] = mb_act(acc[e], a.act);
    const u32x4 o = pack16<T>(acc);
    st16((T*)a.out + (((size_t)b * a.Ho + gy) * a.Wo + gx) * a.C + (size_t)(gv0 + cv) * CE, o);
    if (a.pool) {                      // the pool of the tensor as stored (bf16: after rounding)
      float r[CE];
      unpack16<T>(o, r);
#pragma unroll
      for (int e = 0; e < CE; ++e) psum[e] += r[e];
    }
  }
  if (!a.pool) return;
  // fixed-order reduction over the slots: slot-major partials in LDS (the patch is dead), then one
  // thread per channel adds them in slot order
  __syncthreads();
  float* red = reinterpret_cast<float*>(patch);
#pragma unroll
  for (int e = 0; e < CE; ++e) red[slot * CGC + cv * CE + e] = psum[e];
  __syncthreads();
  if ((int)threadIdx.x < CGC) {
    const int ch = gv0 * CE + threadIdx.x;
    if (ch < a.C) {
      float sum = 0.f;
      for (int q = 0; q < nslots; ++q) sum += red[q * CGC + threadIdx.x];
      a.pool[((size_t)b * gridDim.x + tile) * a.C + ch] = sum;
    }
  }
}

// ---------------------------------------------------------------- SE gate
constexpr int SE_CMAX = 1024, SE_HMAX = 256;

__global__ __launch_bounds__(256) void mb_se_gate_kernel(MbSeArgs a) {
  __shared__ float mean[SE_CMAX];
  __shared__ float hid[SE_HMAX];
  const int b = blockIdx.x, C = a.C, Hd = a.hidden;
  for (int c = threadIdx.x; c < C; c += 256) {
    float s = 0.f;
    for (int t = 0; t < a.tiles; ++t) s += a.pool[((size_t)b * a.tiles + t) * C + c];
    mean[c] = s * a.inv_hw;
  }
  __syncthreads();
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int j = wv; j < Hd; j += 4) {
    float p = 0.f;
#pragma unroll 4
    for (int c = lane; c < C; c += 64) p = fmaf(a.w1[(size_t)j * C + c], mean[c], p);
    p = wave_sum(p);
    if (lane == 0) hid[j] = fmaxf(p + a.b1[j], 0.f);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float p = 0.f;
#pragma unroll 8
    for (int j = 0; j < Hd; ++j) p = fmaf(a.w2t[(size_t)j * C + c], hid[j], p);   // (loads of 8 rows in flight)
    if (a.b2) p += a.b2[c];
    a.scale[(size_t)b * C + c] = fminf(fmaxf(p + 3.f, 0.f), 6.f) / 6.f;
  }
}

// ---------------------------------------------------------------- pointwise / implicit-GEMM conv
constexpr int PW_BM = 64, PW_BN = 64, PW_ROWB = 128;   // tile, bytes of K per row and stage
constexpr int PW_EPI_LD = PW_BN + 4;

SPE_DEV int pw_swz(int row, int chunk) { return row * PW_ROWB + ((chunk ^ (row & 7)) << 4); }

template <typename T>
__global__ __launch_bounds__(256) void mb_gemm_kernel(MbGemmArgs g) {
  constexpr int CE = Chunk<T>::CE, KC = PW_ROWB / (int)sizeof(T);
  __shared__ __attribute__((aligned(16))) char lds[PW_BM * PW_EPI_LD * 4];   // the stage's A + B (16 KB), then the fp32 tile
  char* sa = lds;
  char* sb = lds + PW_BM * PW_ROWB;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int m0 = blockIdx.x * PW_BM, n0 = blockIdx.y * PW_BN;
  const int chunk = tid & 7;
  // the two A rows / W rows this thread stages (rows tid >> 3 and + 32)
  int a_b[2], a_y[2], a_x[2];
  bool a_ok[2];
  const int HoWo = g.Ho * g.Wo;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + (tid >> 3) + 32 * i;
    a_ok[i] = m < g.M;
    const int mm = a_ok[i] ? m : 0;
    a_b[i] = mm / HoWo;
    const int r = mm - a_b[i] * HoWo;
    a_y[i] = (r / g.Wo) * g.stride - g.pad;
    a_x[i] = (r % g.Wo) * g.stride - g.pad;
  }
  u32x4 ra[2], rb[2];
  auto load = [&](int k0) {
    const int k = k0 + chunk * CE;
    const bool kok = k < g.K;
    int tap = 0, ci = k;
    if (g.KH * g.KW > 1) { tap = k / g.Cin; ci = k - tap * g.Cin; }
    const int kh = tap / g.KW, kw = tap - kh * g.KW;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      u32x4 v{0u, 0u, 0u, 0u};
      const int iy = a_y[i] + kh, ix = a_x[i] + kw;
      if (kok && a_ok[i] && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) {
        v = ld16((const T*)g.A + (((size_t)a_b[i] * g.H + iy) * g.W + ix) * g.lda + ci);
        if (g.scale) {
          float x[CE];
          unpack16<T>(v, x);
          const float* sc = g.scale + (size_t)a_b[i] * g.K + k;
#pragma unroll
          for (int e = 0; e < CE; ++e) x[e] *= sc[e];
          v = pack16<T>(x);
        }
      }
      ra[i] = v;
      const int n = n0 + (tid >> 3) + 32 * i;
      rb[i] = (kok && n < g.N) ? ld16((const T*)g.Bw + (size_t)n * g.ldb + k) : u32x4{0u, 0u, 0u, 0u};
    }
  };
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int gq = lane >> 4, rr = lane & 15;
  load(0);
  for (int k0 = 0; k0 < g.K; k0 += KC) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (tid >> 3) + 32 * i;
      st16(sa + pw_swz(row, chunk), ra[i]);
      st16(sb + pw_swz(row, chunk), rb[i]);
    }
    __syncthreads();
    if (k0 + KC < g.K) load(k0 + KC);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const u32x4 av = ld16(sa + pw_swz(wv * 16 + rr, 4 * h + gq));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u32x4 bv = ld16(sb + pw_swz(j * 16 + rr, 4 * h + gq));
        if constexpr (sizeof(T) == 2) {
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv),
                                                           acc[j], 0, 0, 0);
        } else {
          const f32x4 fa = __builtin_bit_cast(f32x4, av), fb = __builtin_bit_cast(f32x4, bv);
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[q], fb[q], acc[j], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  // accumulators -> LDS (row 16 wv + 4 gq + r, column 16 j + rr), then 16 columns of one row a thread
  float* ct = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) ct[(wv * 16 + gq * 4 + r) * PW_EPI_LD + j * 16 + rr] = acc[j][r];
  __syncthreads();
  const int row = tid >> 2, m = m0 + row;
  if (m >= g.M) return;
#pragma unroll
  for (int c8 = 0; c8 < 16; c8 += CE) {
    const int col = (tid & 3) * 16 + c8, n = n0 + col;
    if (n >= g.N) break;
    float v[CE], r[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) v[e] = ct[row * PW_EPI_LD + col + e] + (g.bias ? g.bias[n + e] : 0.f);
    if (g.R) {
      unpack16<T>(ld16((const T*)g.R + (size_t)m * g.ldr + n), r);
#pragma unroll
      for (int e = 0; e < CE; ++e) v[e] += r[e];
    }
#pragma unroll
    for (int e = 0; e < CE; ++e) v[e] = mb_act(v[e], g.act);
    st16((T*)g.C + (size_t)m * g.ldc + n, pack16<T>(v));
  }
}

// NHWC T -> NCHW fp32 (the backbone test hook's output form)
template <typename T>
__global__ void mb_to_nchw_kernel(const T* __restrict__ in, float* __restrict__ out, int HW, int C, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int p = (int)(i % HW), c = (int)((i / HW) % C);
  const size_t b = i / ((size_t)HW * C);
  out[i] = to_f32(in[(b * HW + p) * C + c]);
}

int launch_rc() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

int spe_launch_mb_stem(const ImageSrc& src, const float* w, const float* bias, void* out, int B, int S, int dtype,
                       hipStream_t s) {
  if (src.u8) {
    if (!w || !bias || !out || !stem_u8_fits(src.u8, src.ch, B, S)) return -1;
    const dim3 grid((unsigned)((S / 2 / SU_T) * (S / 2 / SU_T)), (unsigned)B);
    const bool bf = dtype == SPE_DTYPE_BF16;
    if (src.ch == 1) {
      if (bf) mb_stem_u8_kernel<bf16, 1><<<grid, 256, 0, s>>>(src.u8, w, bias, (bf16*)out, S);
      else mb_stem_u8_kernel<float, 1><<<grid, 256, 0, s>>>(src.u8, w, bias, (float*)out, S);
    } else {
      if (bf) mb_stem_u8_kernel<bf16, 3><<<grid, 256, 0, s>>>(src.u8, w, bias, (bf16*)out, S);
      else mb_stem_u8_kernel<float, 3><<<grid, 256, 0, s>>>(src.u8, w, bias, (float*)out, S);
    }
    return launch_rc();
  }
  const float* images = src.f32;
  if (!images || !w || !bias || !out || B <= 0 || S < 2 || (S & 1)) return -1;
  const size_t pix = (size_t)B * (S / 2) * (S / 2);
  const unsigned grid = (unsigned)((pix + 255) / 256);
  if (dtype == SPE_DTYPE_BF16) mb_stem_kernel<bf16><<<grid, 256, 0, s>>>(images, w, bias, (bf16*)out, B, S);
  else mb_stem_kernel<float><<<grid, 256, 0, s>>>(images, w, bias, (float*)out, B, S);
  return launch_rc();
}

int spe_mb_dwconv_tiles(int Ho, int Wo) { return ((Ho + DW_T - 1) / DW_T) * ((Wo + DW_T - 1) / DW_T); }

bool spe_mb_dwconv_fits(int B, int H, int W, int C, int k, int stride) {
  if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || C <= 0 || (C & 7)) return false;
  if (k != 3 && k != 5) return false;
  if (stride == 2) return !(H & 1) && !(W & 1);
  return stride == 1;
}

int spe_launch_mb_dwconv(MbDwArgs a, int dtype, hipStream_t s) {
  if (!a.in || !a.out || !a.w || !a.bias || !spe_mb_dwconv_fits(a.B, a.H, a.W, a.C, a.k, a.stride)) return -1;
  if (a.act != MB_ACT_NONE && a.act != MB_ACT_RELU && a.act != MB_ACT_HSWISH) return -1;
  a.Ho = a.H / a.stride;
  a.Wo = a.W / a.stride;
  const int CE = dtype == SPE_DTYPE_BF16 ? 8 : 4, nvec = a.C / CE;
  int cg = 1;
  while (cg < DW_CGMAX && cg < nvec) cg <<= 1;
  a.cg = cg;
  const dim3 grid((unsigned)spe_mb_dwconv_tiles(a.Ho, a.Wo), (unsigned)((nvec + cg - 1) / cg), (unsigned)a.B);
  if (dtype == SPE_DTYPE_BF16) mb_dwconv_kernel<bf16><<<grid, 256, 0, s>>>(a);
  else mb_dwconv_kernel<float><<<grid, 256, 0, s>>>(a);
  return launch_rc();
}

int spe_launch_mb_se_gate(const MbSeArgs& a, hipStream_t s) {
  if (!a.pool || !a.w1 || !a.b1 || !a.w2t || !a.scale || a.B <= 0 || a.C <= 0 || a.C > SE_CMAX || a.hidden <= 0 ||
      a.hidden > SE_HMAX || a.tiles <= 0)
    return -1;
  mb_se_gate_kernel<<<(unsigned)a.B, 256, 0, s>>>(a);
  return launch_rc();
}

bool spe_mb_gemm_fits(const MbGemmArgs& g) {
  if (g.M <= 0 || g.N <= 0 || g.K <= 0 || (g.N & 7) || (g.K & 7) || (g.Cin & 7) || (g.lda & 7) || (g.ldb & 7) ||
      (g.ldc & 7) || g.ldb < g.K || g.ldc < g.N)
    return false;
  if (g.R && ((g.ldr & 7) || g.ldr < g.N)) return false;
  if (g.KH <= 0 || g.KW <= 0 || g.stride <= 0 || g.pad < 0 || g.K != g.KH * g.KW * g.Cin || g.lda < g.Cin) return false;
  if (g.H <= 0 || g.W <= 0 || g.Ho <= 0 || g.Wo <= 0 || g.M % (g.Ho * g.Wo)) return false;
  if ((g.Ho - 1) * g.stride - g.pad >= g.H || (g.Wo - 1) * g.stride - g.pad >= g.W) return false;
  if (g.scale && g.KH * g.KW != 1) return false;
  return g.act == MB_ACT_NONE || g.act == MB_ACT_RELU || g.act == MB_ACT_HSWISH;
}

int spe_launch_mb_gemm(const MbGemmArgs& g, int dtype, hipStream_t s) {
  if (!g.A || !g.Bw || !g.C || !spe_mb_gemm_fits(g)) return -1;
  const dim3 grid((unsigned)((g.M + PW_BM - 1) / PW_BM), (unsigned)((g.N + PW_BN - 1) / PW_BN));
  if (dtype == SPE_DTYPE_BF16) mb_gemm_kernel<bf16><<<grid, 256, 0, s>>>(g);
  else mb_gemm_kernel<float><<<grid, 256, 0, s>>>(g);
  return launch_rc();
}

int spe_launch_mb_to_nchw(const void* in, float* out, int B, int HW, int C, int dtype, hipStream_t s) {
  const size_t total = (size_t)B * HW * C;
  const unsigned grid = (unsigned)((total + 255) / 256);
  if (dtype == SPE_DTYPE_BF16) mb_to_nchw_kernel<bf16><<<grid, 256, 0, s>>>((const bf16*)in, out, HW, C, total);
  else mb_to_nchw_kernel<float><<<grid, 256, 0, s>>>((const float*)in, out, HW, C, total);
  return launch_rc();
}
