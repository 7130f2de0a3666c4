// GhostNetV2 backbone kernels of the UNC RT-DETR model (UNC/nn/backbone/ghostnetv2.py:88-441), gfx950,
// NHWC, storage T = bf16 or float, fp32 accumulation, 16-byte channel vectors, no floating-point atomics:
//
//   gh_stem    conv_stem 3x3/s2 3 -> 16 from the fp32 NCHW batch, two outputs: the raw conv output (what
//              the 64 x 64 resize and Conv1 read) and relu(bn1(.)) (what the blocks read); gh_stem_u8: the
//              same from the 8-bit crops the batch is normalised from, tiled through LDS
//   gh_cheap   the ghost module's second half and what follows it: x2 = act(dw3x3(x1) + bias) over an
//              8 x 8 tile x a group of channel vectors, x1 (a channel slice of a wider tensor) staged with
//              its halo in LDS; writes out[:half] = post(x1), out[half:] = post(x2), post = nothing, the
//              DFC gate (gate[b][h/2][w/2][c], nearest x2 upsampling: applied AFTER the cheap op, which
//              reads the ungated x1) or the residual add (ghost2, no activation); optionally the per-tile
//              per-channel sums of the stored outputs in a fixed order ([B][tiles][2 half], mb_se_gate's
//              input)
//   gh_dfc     the DFC attention branch after its 1x1 conv: depthwise 1x5 (pad 0,2) + bias -> depthwise 5x1
//              (pad 2,0) + bias -> sigmoid; the whole pooled map (<= 32 x 32) of a group of channel vectors
//              in LDS; the two passes are evaluated together per output (25 taps, the intermediate never
//              rounded, zero outside the map as the reference pads it)
//   gh_pool2   2x2 mean in front of the DFC branch's 1x1 conv
//
// Widths: every half width is a multiple of 8 here.  The model pads a ghost half to the next multiple of 8
// with zero weights and biases, so a pad lane holds exactly 0 through ReLU, gate, residual and pool.
#include <hip/hip_runtime.h>

#include "spe_common.h"
#include "spe_kernels.h"
#include "stem_u8.h"

namespace {

constexpr int GH_T = 8;                       // output tile edge
constexpr int GH_P = GH_T + 2;                 // patch edge (3x3, stride 1)
constexpr int GH_CGMAX = 8;                    // 16-byte channel vectors per work-group
constexpr int GH_LDS = 2 * 256 * 8 * 4;        // the pool reduction's slot-major partials (>= the patch's 12.5 KB)

template <typename T>
__global__ __launch_bounds__(256) void gh_stem_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      T* __restrict__ raw, T* __restrict__ act, int B, int S) {
  __shared__ float wl[27 * 16 + 32];
  for (int i = threadIdx.x; i < 27 * 16 + 32; i += 256) wl[i] = i < 432 ? w[i] : i < 448 ? scale[i - 432] : shift[i - 448];
  __syncthreads();
  const int So = S >> 1;
  const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= (size_t)B * So * So) return;
  const int ox = (int)(pix % So), oy = (int)((pix / So) % So), b = (int)(pix / ((size_t)So * So));
  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = 0.f;
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
  constexpr int CE = Chunk<T>::CE;
#pragma unroll
  for (int c = 0; c < 16; c += CE) st16(raw + pix * 16 + c, pack16<T>(acc + c));
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = fmaxf(fmaf(acc[c], wl[432 + c], wl[448 + c]), 0.f);
#pragma unroll
  for (int c = 0; c < 16; c += CE) st16(act + pix * 16 + c, pack16<T>(acc + c));
}

// the same stem from the 8-bit crops [B][S][S][CH]: a 16 x 16 output tile a work-group, the patch staged and
// normalised once in LDS (stem_u8.h); both outputs bit-identical to gh_stem_kernel's on the batch normalised
// that way
template <typename T, int CH>
__global__ __launch_bounds__(256) void gh_stem_u8_kernel(const uint8_t* __restrict__ crops, const float* __restrict__ w,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         T* __restrict__ raw, T* __restrict__ act, int S) {
  __shared__ float wl[27 * 16 + 32];
  __shared__ StemU8Lds lds;
  for (int i = threadIdx.x; i < 27 * 16 + 32; i += 256) wl[i] = i < 432 ? w[i] : i < 448 ? scale[i - 432] : shift[i - 448];
  const int So = S >> 1, tiles_x = So / SU_T;
  const int ty0 = (blockIdx.x / tiles_x) * SU_T, tx0 = (blockIdx.x % tiles_x) * SU_T, b = blockIdx.y;
  stem_u8_stage<CH>(crops, S, b, ty0, tx0, lds);          // (its barriers cover wl)
  const int ox = threadIdx.x & (SU_T - 1), oy = threadIdx.x / SU_T, gy = ty0 + oy, gx = tx0 + ox;
  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = 0.f;
  stem_u8_accumulate(lds.x, wl, S, gy, gx, oy, ox, acc);
  constexpr int CE = Chunk<T>::CE;
  const size_t pix = ((size_t)b * So + gy) * So + gx;
#pragma unroll
  for (int c = 0; c < 16; c += CE) st16(raw + pix * 16 + c, pack16<T>(acc + c));
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = fmaxf(fmaf(acc[c], wl[432 + c], wl[448 + c]), 0.f);
#pragma unroll
  for (int c = 0; c < 16; c += CE) st16(act + pix * 16 + c, pack16<T>(acc + c));
}

template <typename T>
__global__ __launch_bounds__(256) void gh_cheap_kernel(GhCheapArgs a) {
  constexpr int CE = Chunk<T>::CE;
  __shared__ __attribute__((aligned(16))) char lds[GH_LDS];
  __shared__ float wl[9 * GH_CGMAX * 8];
  u32x4* patch = reinterpret_cast<u32x4*>(lds);
  const int CG = a.cg, CGC = CG * CE, nvec = a.half / CE, C2 = 2 * a.half;
  const int tiles_x = (a.W + GH_T - 1) / GH_T;
  const int tile = blockIdx.x, ty0 = (tile / tiles_x) * GH_T, tx0 = (tile % tiles_x) * GH_T;
  const int gv0 = blockIdx.y * CG, b = blockIdx.z;
  const T* in = (const T*)a.x1 + (size_t)b * a.H * a.W * a.ldx + a.xoff;
  for (int i = threadIdx.x; i < GH_P * GH_P * CG; i += 256) {
    const int cv = i % CG, p = i / CG, py = p / GH_P, px = p - py * GH_P;
    const int iy = ty0 - 1 + py, ix = tx0 - 1 + px;
    u32x4 v{0u, 0u, 0u, 0u};
    if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W && gv0 + cv < nvec)
      v = ld16(in + ((size_t)iy * a.W + ix) * a.ldx + (size_t)(gv0 + cv) * CE);
    patch[i] = v;
  }
  for (int i = threadIdx.x; i < 9 * CGC; i += 256) {
    const int tap = i / CGC, c = i - tap * CGC, ch = gv0 * CE + c;
    wl[i] = ch < a.half ? a.w[(size_t)tap * a.half + ch] : 0.f;
  }
  __syncthreads();
  const int cv = threadIdx.x % CG, slot = threadIdx.x / CG, nslots = 256 / CG;
  const bool cvalid = gv0 + cv < nvec;
  const int ch0 = (gv0 + cv) * CE;
  float bs[CE], ps1[CE], ps2[CE];
#pragma unroll
  for (int e = 0; e < CE; ++e) {
    bs[e] = cvalid ? a.bias[ch0 + e] : 0.f;
    ps1[e] = 0.f;
    ps2[e] = 0.f;
  }
  for (int p = slot; p < GH_T * GH_T; p += nslots) {
    const int oy = p / GH_T, ox = p % GH_T, gy = ty0 + oy, gx = tx0 + ox;
    if (!cvalid || gy >= a.H || gx >= a.W) continue;
    float v1[CE], v2[CE];
    unpack16<T>(patch[((oy + 1) * GH_P + ox + 1) * CG + cv], v1);
#pragma unroll
    for (int e = 0; e < CE; ++e) v2[e] = bs[e];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        float x[CE];
        unpack16<T>(patch[((oy + kh) * GH_P + ox + kw) * CG + cv], x);
        const float* wk = &wl[(kh * 3 + kw) * CGC + cv * CE];
#pragma unroll
        for (int e = 0; e < CE; ++e) v2[e] = fmaf(x[e], wk[e], v2[e]);
      }
    if (a.act == MB_ACT_RELU) {
#pragma unroll
      for (int e = 0; e < CE; ++e) v2[e] = fmaxf(v2[e], 0.f);
    }
    const size_t opix = ((size_t)b * a.H + gy) * a.W + gx;
    if (a.post == GH_POST_GATE) {
      const T* g = (const T*)a.gate + (((size_t)b * (a.H >> 1) + (gy >> 1)) * (a.W >> 1) + (gx >> 1)) * C2 + ch0;
      float g1[CE], g2[CE];
      unpack16<T>(ld16(g), g1);
      unpack16<T>(ld16(g + a.half), g2);
#pragma unroll
      for (int e = 0; e < CE; ++e) { v1[e] *= g1[e]; v2[e] *= g2[e]; }
    } else if (a.post == GH_POST_RESIDUAL) {
      const T* r = (const T*)a.resid + opix * C2 + ch0;
      float r1[CE], r2[CE];
      unpack16<T>(ld16(r), r1);
      unpack16<T>(ld16(r + a.half), r2);
#pragma unroll
      for (int e = 0; e < CE; ++e) { v1[e] += r1[e]; v2[e] += r2[e]; }
    }
    const u32x4 o1 = pack16<T>(v1), o2 = pack16<T>(v2);
    T* o = (T*)a.out + opix * C2 + ch0;
    st16(o, o1);
    st16(o + a.half, o2);
    if (a.pool) {                      // the pool of the tensor as stored (bf16: after rounding)
      unpack16<T>(o1, v1);
      unpack16<T>(o2, v2);
#pragma unroll
      for (int e = 0; e < CE; ++e) { ps1[e] += v1[e]; ps2[e] += v2[e]; }
    }
  }
  if (!a.pool) return;
  // fixed-order reduction over the slots: slot-major partials in LDS (the patch is dead), then one thread
  // per channel of either half adds them in slot order
  __syncthreads();
  float* red = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int e = 0; e < CE; ++e) {
    red[(slot * 2 + 0) * CGC + cv * CE + e] = ps1[e];
    red[(slot * 2 + 1) * CGC + cv * CE + e] = ps2[e];
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * CGC) {
    const int hf = threadIdx.x / CGC, c = threadIdx.x - hf * CGC, ch = gv0 * CE + c;
    if (ch < a.half) {
      float sum = 0.f;
      for (int q = 0; q < nslots; ++q) sum += red[(q * 2 + hf) * CGC + c];
      a.pool[((size_t)b * gridDim.x + tile) * C2 + hf * a.half + ch] = sum;
    }
  }
}

constexpr int DFC_MAX = 32;                    // largest pooled map edge
constexpr int DFC_ITEMS = DFC_MAX * DFC_MAX;   // (pixel, channel vector) pairs per work-group

template <typename T>
__global__ __launch_bounds__(256) void gh_dfc_kernel(GhDfcArgs a) {
  constexpr int CE = Chunk<T>::CE;
  __shared__ u32x4 map[DFC_ITEMS];
  const int CG = a.cg, HW = a.H * a.W, nvec = a.C / CE;
  const int gv0 = blockIdx.x * CG, b = blockIdx.y;
  const T* in = (const T*)a.x + (size_t)b * HW * a.C;
  for (int i = threadIdx.x; i < HW * CG; i += 256) {
    const int cv = i % CG, p = i / CG;
    map[i] = gv0 + cv < nvec ? ld16(in + (size_t)p * a.C + (size_t)(gv0 + cv) * CE) : u32x4{0u, 0u, 0u, 0u};
  }
  __syncthreads();
  for (int i = threadIdx.x; i < HW * CG; i += 256) {
    const int cv = i % CG, p = i / CG, y = p / a.W, x = p - y * a.W;
    if (gv0 + cv >= nvec) continue;
    const int ch0 = (gv0 + cv) * CE;
    float acc[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) acc[e] = a.b2[ch0 + e];
    for (int dy = -2; dy <= 2; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy >= a.H) continue;         // the 5x1 conv pads the 1x5 conv's OUTPUT with zeros
      float row[CE];
#pragma unroll
      for (int e = 0; e < CE; ++e) row[e] = a.b1[ch0 + e];
      for (int dx = -2; dx <= 2; ++dx) {
        const int xx = x + dx;
        if (xx < 0 || xx >= a.W) continue;
        float v[CE];
        unpack16<T>(map[(yy * a.W + xx) * CG + cv], v);
        const float* wk = a.w1 + (size_t)(dx + 2) * a.C + ch0;
#pragma unroll
        for (int e = 0; e < CE; ++e) row[e] = fmaf(v[e], wk[e], row[e]);
      }
      const float* wk = a.w2 + (size_t)(dy + 2) * a.C + ch0;
#pragma unroll
      for (int e = 0; e < CE; ++e) acc[e] = fmaf(row[e], wk[e], acc[e]);
    }
#pragma unroll
    for (int e = 0; e < CE; ++e) acc[e] = 1.f / (1.f + expf(-acc[e]));
    st16((T*)a.gate + ((size_t)b * HW + p) * a.C + ch0, pack16<T>(acc));
  }
}

template <typename T>
__global__ __launch_bounds__(256) void gh_pool2_kernel(const T* __restrict__ in, T* __restrict__ out, int H, int W, int C,
                                                       size_t total) {
  constexpr int CE = Chunk<T>::CE;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int nvec = C / CE, Wo = W >> 1, Ho = H >> 1;
  const int cv = (int)(i % nvec), ox = (int)((i / nvec) % Wo), oy = (int)((i / ((size_t)nvec * Wo)) % Ho);
  const size_t b = i / ((size_t)nvec * Wo * Ho);
  const T* p = in + ((b * H + 2 * oy) * W + 2 * ox) * C + (size_t)cv * CE;
  float s[CE], v[CE];
  unpack16<T>(ld16(p), s);
  unpack16<T>(ld16(p + C), v);
#pragma unroll
  for (int e = 0; e < CE; ++e) s[e] += v[e];
  unpack16<T>(ld16(p + (size_t)W * C), v);
#pragma unroll
  for (int e = 0; e < CE; ++e) s[e] += v[e];
  unpack16<T>(ld16(p + (size_t)W * C + C), v);
#pragma unroll
  for (int e = 0; e < CE; ++e) s[e] = (s[e] + v[e]) * 0.25f;
  st16(out + ((b * Ho + oy) * Wo + ox) * C + (size_t)cv * CE, pack16<T>(s));
}

int launch_rc() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

int pow2_vecs(int nvec, int cap) {
  int cg = 1;
  while (cg < cap && cg < nvec) cg <<= 1;
  return cg;
}

}  // namespace

int spe_launch_gh_stem(const ImageSrc& src, const float* w, const float* scale, const float* shift, void* raw, void* act,
                       int B, int S, int dtype, hipStream_t s) {
  if (src.u8) {
    if (!w || !scale || !shift || !raw || !act || !stem_u8_fits(src.u8, src.ch, B, S)) return -1;
    const dim3 grid((unsigned)((S / 2 / SU_T) * (S / 2 / SU_T)), (unsigned)B);
    const bool bf = dtype == SPE_DTYPE_BF16;
    if (src.ch == 1) {
      if (bf) gh_stem_u8_kernel<bf16, 1><<<grid, 256, 0, s>>>(src.u8, w, scale, shift, (bf16*)raw, (bf16*)act, S);
      else gh_stem_u8_kernel<float, 1><<<grid, 256, 0, s>>>(src.u8, w, scale, shift, (float*)raw, (float*)act, S);
    } else {
      if (bf) gh_stem_u8_kernel<bf16, 3><<<grid, 256, 0, s>>>(src.u8, w, scale, shift, (bf16*)raw, (bf16*)act, S);
      else gh_stem_u8_kernel<float, 3><<<grid, 256, 0, s>>>(src.u8, w, scale, shift, (float*)raw, (float*)act, S);
    }
    return launch_rc();
  }
  const float* images = src.f32;
  if (!images || !w || !scale || !shift || !raw || !act || B <= 0 || S < 2 || (S & 1)) return -1;
  const size_t pix = (size_t)B * (S / 2) * (S / 2);
  const unsigned grid = (unsigned)((pix + 255) / 256);
  if (dtype == SPE_DTYPE_BF16) gh_stem_kernel<bf16><<<grid, 256, 0, s>>>(images, w, scale, shift, (bf16*)raw, (bf16*)act, B, S);
  else gh_stem_kernel<float><<<grid, 256, 0, s>>>(images, w, scale, shift, (float*)raw, (float*)act, B, S);
  return launch_rc();
}

int spe_gh_cheap_tiles(int H, int W) { return ((H + GH_T - 1) / GH_T) * ((W + GH_T - 1) / GH_T); }

bool spe_gh_cheap_fits(const GhCheapArgs& a) {
  if (a.B <= 0 || a.B > 65535 || a.H <= 0 || a.W <= 0 || a.half <= 0 || (a.half & 7)) return false;
  if ((a.ldx & 7) || (a.xoff & 7) || a.xoff < 0 || a.ldx < a.xoff + a.half) return false;
  if (a.act != MB_ACT_NONE && a.act != MB_ACT_RELU) return false;
  if (a.post != GH_POST_NONE && a.post != GH_POST_GATE && a.post != GH_POST_RESIDUAL) return false;
  if (a.post == GH_POST_GATE && ((a.H & 1) || (a.W & 1))) return false;
  return true;
}

int spe_launch_gh_cheap(GhCheapArgs a, int dtype, hipStream_t s) {
  if (!a.x1 || !a.w || !a.bias || !a.out || !spe_gh_cheap_fits(a)) return -1;
  if ((a.post == GH_POST_GATE && !a.gate) || (a.post == GH_POST_RESIDUAL && !a.resid)) return -1;
  const int CE = dtype == SPE_DTYPE_BF16 ? 8 : 4, nvec = a.half / CE;
  a.cg = pow2_vecs(nvec, GH_CGMAX);
  const dim3 grid((unsigned)spe_gh_cheap_tiles(a.H, a.W), (unsigned)((nvec + a.cg - 1) / a.cg), (unsigned)a.B);
  if (dtype == SPE_DTYPE_BF16) gh_cheap_kernel<bf16><<<grid, 256, 0, s>>>(a);
  else gh_cheap_kernel<float><<<grid, 256, 0, s>>>(a);
  return launch_rc();
}

bool spe_gh_dfc_fits(int B, int H, int W, int C) {
  return B > 0 && B <= 65535 && H > 0 && W > 0 && H <= DFC_MAX && W <= DFC_MAX && C > 0 && !(C & 7);
}

int spe_launch_gh_dfc(GhDfcArgs a, int dtype, hipStream_t s) {
  if (!a.x || !a.w1 || !a.b1 || !a.w2 || !a.b2 || !a.gate || !spe_gh_dfc_fits(a.B, a.H, a.W, a.C)) return -1;
  const int CE = dtype == SPE_DTYPE_BF16 ? 8 : 4, nvec = a.C / CE;
  int cap = DFC_ITEMS / (a.H * a.W);
  if (cap > GH_CGMAX) cap = GH_CGMAX;
  int cg = 1;
  while (cg * 2 <= cap && cg < nvec) cg <<= 1;
  a.cg = cg;
  const dim3 grid((unsigned)((nvec + cg - 1) / cg), (unsigned)a.B);
  if (dtype == SPE_DTYPE_BF16) gh_dfc_kernel<bf16><<<grid, 256, 0, s>>>(a);
  else gh_dfc_kernel<float><<<grid, 256, 0, s>>>(a);
  return launch_rc();
}

bool spe_gh_pool2_fits(int B, int H, int W, int C) {
  return B > 0 && H > 0 && W > 0 && !(H & 1) && !(W & 1) && C > 0 && !(C & 7);
}

int spe_launch_gh_pool2(const void* in, void* out, int B, int H, int W, int C, int dtype, hipStream_t s) {
  if (!in || !out || !spe_gh_pool2_fits(B, H, W, C)) return -1;
  const int CE = dtype == SPE_DTYPE_BF16 ? 8 : 4;
  const size_t total = (size_t)B * (H / 2) * (W / 2) * (C / CE);
  const unsigned grid = (unsigned)((total + 255) / 256);
  if (dtype == SPE_DTYPE_BF16) gh_pool2_kernel<bf16><<<grid, 256, 0, s>>>((const bf16*)in, (bf16*)out, H, W, C, total);
  else gh_pool2_kernel<float><<<grid, 256, 0, s>>>((const float*)in, (float*)out, H, W, C, total);
  return launch_rc();
}
