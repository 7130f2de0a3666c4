// MobileNetV3_Small entry of the UNC RT-DETR model (UNC/nn/backbone/mobilenetv3.py:228-320), gfx950, NHWC,
// storage T = bf16 or float.
//
//   mbs_entry    from the image (the fp32 NCHW batch, or the 8-bit crops through stem_u8.h's normalisation) to
//                the three S/4 x S/4 x 16 maps everything behind the stem reads, without storing the S/2 x S/2
//                stem map or block 0's expanded tensor:
//                  pooled = the 2 x 2 mean of hswish(bn1(conv1 3x3/s2)): F.interpolate(.., (64, 64)) at 256,
//                           Conv1's input
//                  skip   = bn(dw3x3/s2(stem)): block 0's skip (stride 2, in == out)
//                  t2     = relu(bn2(dw3x3/s2(relu(bn1(conv1x1 16 -> 16(stem)))))): block 0's depthwise output,
//                           with its SE pool partials in mb_dwconv's layout [B][tiles][16]
//
// One work-group of 256 threads owns an 8 x 8 output tile of one image.  Its 35 x 35 x 3 image patch is staged
// in LDS as fp32, the 17 x 17 x 16 stem patch (one halo row above, one halo column to the left) is computed
// from it into LDS, the expanded patch of the same shape takes the image patch's place, and the three outputs
// are 2 x 2 / 3 x 3 stencils over the two patches.  Outside the S/2 x S/2 map both patches are ZERO (the
// reference pads the stem map and the expanded map, it does not extend them by act(bias)).  Everything stays
// fp32 until each output is rounded once to T; the pool partials sum the values as stored, one thread a
// channel in pixel order (no floating-point atomics).  LDS: 1040 + 2 * 4624 floats = 41 152 bytes, three
// work-groups a CU.  K = 27 / 16 / 9 a value: VALU work, the point is bytes and launches.
#include <hip/hip_runtime.h>

#include "spe_common.h"
#include "spe_kernels.h"
#include "stem_u8.h"

namespace {

constexpr int ME_T = 8;                      // output tile edge
constexpr int ME_SP = 2 * ME_T + 1;          // stem / expanded patch edge (17)
constexpr int ME_IP = 2 * ME_SP + 1;         // image patch edge (35)
constexpr int ME_IPW = ME_IP + 1;            // floats per image patch row
constexpr int ME_IPL = ME_IP * ME_IPW;       // floats per image patch plane
constexpr int ME_PATCH = ME_SP * ME_SP * 16; // floats per stem / expanded patch
static_assert(3 * ME_IPL <= ME_PATCH, "the image patch lives where the expanded patch is written later");
static_assert(ME_T * ME_T * 16 <= ME_PATCH, "so do the pool partials");

SPE_DEV float me_hswish(float v) { return v * fminf(fmaxf(v + 3.f, 0.f), 6.f) / 6.f; }

// CH 0: the fp32 NCHW batch; 1 / 3: 8-bit crops [B][S][S][CH]
template <typename T, int CH>
__global__ __launch_bounds__(256) void mbs_entry_kernel(MbsEntryArgs a) {
  __shared__ __attribute__((aligned(16))) float wl[MBS_W_FLOATS];
  __shared__ __attribute__((aligned(16))) float stem[ME_PATCH];
  __shared__ __attribute__((aligned(16))) float ub[ME_PATCH];    // image patch, then expanded patch, then pool rows
  const int S = a.S, H1 = S >> 1, G = S >> 2;
  const int tiles_x = (G + ME_T - 1) / ME_T;
  const int tile = blockIdx.x, ty0 = (tile / tiles_x) * ME_T, tx0 = (tile % tiles_x) * ME_T, b = blockIdx.y;
  const int tid = threadIdx.x;
  for (int i = tid; i < MBS_W_FLOATS; i += 256) wl[i] = a.w[i];
  // image patch: rows 4 ty0 - 3 .. 4 ty0 + 31, zero outside the frame
  const int iy0 = 4 * ty0 - 3, ix0 = 4 * tx0 - 3;
  for (int i = tid; i < ME_IP * ME_IP; i += 256) {
    const int py = i / ME_IP, px = i - py * ME_IP, iy = iy0 + py, ix = ix0 + px;
    float v[3] = {0.f, 0.f, 0.f};
    if (iy >= 0 && iy < S && ix >= 0 && ix < S) {
      if constexpr (CH == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = a.src.f32[(((size_t)b * 3 + c) * S + iy) * S + ix];
      } else {
        const uint8_t* u = a.src.u8 + (((size_t)b * S + iy) * S + ix) * CH;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = stem_u8_norm(u[CH == 1 ? 0 : c], c);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) ub[c * ME_IPL + py * ME_IPW + px] = v[c];
  }
  __syncthreads();
  // stem patch: position (sy, sx) <-> stem pixel (2 ty0 - 1 + sy, 2 tx0 - 1 + sx), four channels an item;
  // its taps are image patch rows 2 sy + kh, columns 2 sx + kw (out-of-frame taps are zeros there)
  for (int it = tid; it < ME_SP * ME_SP * 4; it += 256) {
    const int pos = it >> 2, q = it & 3, sy = pos / ME_SP, sx = pos - sy * ME_SP;
    const int gy = 2 * ty0 - 1 + sy, gx = 2 * tx0 - 1 + sx;
    float acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = wl[MBS_W_STEM_B + 4 * q + e];
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const float x = ub[ci * ME_IPL + (2 * sy + kh) * ME_IPW + 2 * sx + kw];
          const float* wk = &wl[MBS_W_STEM + ((ci * 3 + kh) * 3 + kw) * 16 + 4 * q];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = fmaf(x, wk[e], acc[e]);
        }
    const bool in = gy >= 0 && gy < H1 && gx >= 0 && gx < H1;
#pragma unroll
    for (int e = 0; e < 4; ++e) stem[pos * 16 + 4 * q + e] = in ? me_hswish(acc[e]) : 0.f;
  }
  __syncthreads();                     // (the image patch is dead: ub becomes the expanded patch)
  for (int it = tid; it < ME_SP * ME_SP * 4; it += 256) {
    const int pos = it >> 2, q = it & 3, sy = pos / ME_SP, sx = pos - sy * ME_SP;
    const int gy = 2 * ty0 - 1 + sy, gx = 2 * tx0 - 1 + sx;
    float acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = wl[MBS_W_EXP_B + 4 * q + e];
#pragma unroll
    for (int ci = 0; ci < 16; ++ci) {
      const float x = stem[pos * 16 + ci];
      const float* wk = &wl[MBS_W_EXP + ci * 16 + 4 * q];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(x, wk[e], acc[e]);
    }
    const bool in = gy >= 0 && gy < H1 && gx >= 0 && gx < H1;
#pragma unroll
    for (int e = 0; e < 4; ++e) ub[pos * 16 + 4 * q + e] = in ? fmaxf(acc[e], 0.f) : 0.f;
  }
  __syncthreads();
  // outputs: one pixel x four channels a thread; its 3 x 3 window is patch rows 2 oy + kh, columns 2 ox + kw,
  // its 2 x 2 mean rows 2 oy + 1 .. + 2
  const int pix = tid >> 2, q = tid & 3, oy = pix >> 3, ox = pix & 7, gy = ty0 + oy, gx = tx0 + ox;
  const bool valid = gy < G && gx < G;
  float pl[4], sk[4], dw[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    sk[e] = wl[MBS_W_SKIP_B + 4 * q + e];
    dw[e] = wl[MBS_W_DW_B + 4 * q + e];
  }
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int p = ((2 * oy + kh) * ME_SP + 2 * ox + kw) * 16 + 4 * q, t = (kh * 3 + kw) * 16 + 4 * q;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sk[e] = fmaf(stem[p + e], wl[MBS_W_SKIP + t + e], sk[e]);
        dw[e] = fmaf(ub[p + e], wl[MBS_W_DW + t + e], dw[e]);
      }
    }
  {
    const int p = ((2 * oy + 1) * ME_SP + 2 * ox + 1) * 16 + 4 * q;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      pl[e] = 0.25f * ((stem[p + e] + stem[p + 16 + e]) + (stem[p + ME_SP * 16 + e] + stem[p + ME_SP * 16 + 16 + e]));
  }
  float stored[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    dw[e] = fmaxf(dw[e], 0.f);
    stored[e] = to_f32(from_f32<T>(dw[e]));
  }
  if (valid) {
    const size_t o = (((size_t)b * G + gy) * G + gx) * 16 + 4 * q;
    if constexpr (sizeof(T) == 4) {
      st16((T*)a.pooled + o, pack16<float>(pl));
      st16((T*)a.skip + o, pack16<float>(sk));
      st16((T*)a.t2 + o, pack16<float>(dw));
    } else {
      st8((T*)a.pooled + o, u32x2{pack_bf16x2(pl[0], pl[1]), pack_bf16x2(pl[2], pl[3])});
      st8((T*)a.skip + o, u32x2{pack_bf16x2(sk[0], sk[1]), pack_bf16x2(sk[2], sk[3])});
      st8((T*)a.t2 + o, u32x2{pack_bf16x2(dw[0], dw[1]), pack_bf16x2(dw[2], dw[3])});
    }
  }
  // SE pool partials of t2 as stored: pixel-major rows in LDS (both patches are dead), one thread a channel
  // adds them in pixel order
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e) ub[pix * 16 + 4 * q + e] = valid ? stored[e] : 0.f;
  __syncthreads();
  if (a.pool && tid < 16) {
    float sum = 0.f;
    for (int p = 0; p < ME_T * ME_T; ++p) sum += ub[p * 16 + tid];
    a.pool[((size_t)b * gridDim.x + tile) * 16 + tid] = sum;
  }
}

template <typename T>
void mbs_launch(const MbsEntryArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)spe_mbs_entry_tiles(a.S), (unsigned)a.B);
  if (!a.src.u8) mbs_entry_kernel<T, 0><<<grid, 256, 0, s>>>(a);
  else if (a.src.ch == 1) mbs_entry_kernel<T, 1><<<grid, 256, 0, s>>>(a);
  else mbs_entry_kernel<T, 3><<<grid, 256, 0, s>>>(a);
}

}  // namespace

bool spe_mbs_entry_enabled() {
  static const int on = spe_env_int("SPE_MBS_ENTRY", 1);
  return on != 0;
}

bool spe_mbs_entry_fits(int B, int S) { return B > 0 && B <= 65535 && S >= 32 && S <= 4096 && S % 16 == 0; }

int spe_mbs_entry_tiles(int S) {
  const int t = (S / 4 + ME_T - 1) / ME_T;
  return t * t;
}

int spe_launch_mbs_entry(const MbsEntryArgs& a, int dtype, hipStream_t s) {
  if (!a.w || !a.pooled || !a.skip || !a.t2 || !spe_mbs_entry_fits(a.B, a.S)) return -1;
  if (a.src.u8 ? (a.src.ch != 1 && a.src.ch != 3) : !a.src.f32) return -1;
  if (dtype == SPE_DTYPE_BF16) mbs_launch<bf16>(a, s);
  else mbs_launch<float>(a, s);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
