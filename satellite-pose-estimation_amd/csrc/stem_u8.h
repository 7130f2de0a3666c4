// 8-bit ingest of the two light backbones' stems (mbv3.hip mb_stem_u8, ghostv2.hip gh_stem_u8): the 3x3 /
// stride 2 / pad 1, 3 -> 16 convolution read from the u8 crops [B][S][S][CH] (CH 1 gray, 3 RGB) instead of
// the fp32 NCHW batch normalised from them.
//
// One work-group of 256 threads owns a 16 x 16 output tile, one output pixel a thread.  Its 33 x 33 input
// patch (stride 2, one halo row above and one halo column to the left) arrives as whole dwords, row by row
// (a row's 1 + 8 CH dwords are contiguous: coalesced), is kept as bytes in LDS, and every pixel is normalised
// ONCE into fp32 in LDS -- ((float)u / 255.f - mean[c]) / std[c] with IEEE division, the operation order of
// SrcU8 (elementwise.hip), a gray byte feeding all three channels.  The fp32 kernels normalise nothing but
// read every pixel 2.25 times through 27 strided 4-byte loads a thread.  The accumulation then walks ci, kh,
// kw in the fp32 kernels' order with the same fmaf chain and the same skipped out-of-frame taps, so the result
// is bit-identical to the fp32 kernel fed the batch normalised that way.
//
// LDS plane layout: a patch row holds its even columns, then its odd columns (SU_HALF floats each), so the 16
// pixels of a tile row read consecutive floats for every tap (column 2 ox + kw) instead of every other one.
#pragma once
#include "spe_common.h"

constexpr int SU_T = 16;                   // output tile edge
constexpr int SU_P = 2 * SU_T + 1;         // input patch edge
constexpr int SU_HALF = SU_T + 1;          // patch columns of one parity
constexpr int SU_ROW = 2 * SU_HALF;        // floats per patch row
constexpr int SU_PLANE = SU_P * SU_ROW;    // floats per channel plane
constexpr int SU_RAW_DW = 1 + 8 * 3;       // dwords per raw patch row at CH = 3

struct StemU8Lds {
  uint32_t raw[SU_P * SU_RAW_DW];          // the patch's bytes: row py starts 4 bytes left of column 1
  float x[3 * SU_PLANE];                   // the normalised patch, [c][py][parity][column / 2]
};

// One crop byte as channel c of the normalised batch: the expression stem_u8_stage evaluates, for kernels that
// stage a patch of their own (mbv3s.hip)
SPE_DEV float stem_u8_norm(uint8_t u, int c) {
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  return ((float)u / 255.f - mean[c]) / stdv[c];
}

// Stage and normalise the patch of output tile (ty0, tx0) of image b.  Every thread of the work-group calls
// it; the patch is complete on return.  Needs S % (2 SU_T) == 0 and crops 4-byte aligned (the launchers check).
template <int CH>
SPE_DEV void stem_u8_stage(const uint8_t* __restrict__ crops, int S, int b, int ty0, int tx0, StemU8Lds& l) {
  constexpr int NDW = 1 + 8 * CH;
  const int rowb = S * CH;                                  // bytes per image row
  const int col0 = 2 * tx0 * CH - 4;                        // byte offset of a raw row's first dword in its image row
  const uint8_t* img = crops + (size_t)b * S * rowb;
  for (int i = threadIdx.x; i < SU_P * NDW; i += 256) {
    const int py = i / NDW, j = i - py * NDW;
    const int iy = 2 * ty0 - 1 + py, off = col0 + 4 * j;
    uint32_t v = 0u;
    if (iy >= 0 && iy < S && off >= 0 && off + 4 <= rowb)
      v = *reinterpret_cast<const uint32_t*>(img + (size_t)iy * rowb + off);
    l.raw[py * NDW + j] = v;
  }
  __syncthreads();
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  const uint8_t* rawb = reinterpret_cast<const uint8_t*>(l.raw);
  for (int i = threadIdx.x; i < SU_P * SU_P; i += 256) {
    const int py = i / SU_P, px = i - py * SU_P;
    const int iy = 2 * ty0 - 1 + py, ix = 2 * tx0 - 1 + px;
    const bool in = iy >= 0 && iy < S && ix >= 0 && ix < S;
    const uint8_t* u = rawb + py * NDW * 4 + 4 + (px - 1) * CH;
    float* o = l.x + py * SU_ROW + (px & 1) * SU_HALF + (px >> 1);
    if constexpr (CH == 1) {
      const float q = (float)u[0] / 255.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c * SU_PLANE] = in ? (q - mean[c]) / stdv[c] : 0.f;
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c * SU_PLANE] = in ? ((float)u[c] / 255.f - mean[c]) / stdv[c] : 0.f;
    }
  }
  __syncthreads();
}

// acc[c] += sum over the taps of output pixel (gy, gx) (tile-local (oy, ox)), in the fp32 stems' order:
// ci outer, kh, kw, one fmaf a tap and channel, an out-of-frame tap skipped.  wl: LDS fp32 [27][16].
SPE_DEV void stem_u8_accumulate(const float* xs, const float* wl, int S, int gy, int gx, int oy, int ox, float acc[16]) {
  for (int ci = 0; ci < 3; ++ci)
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int iy = 2 * gy - 1 + kh;
      if (iy < 0 || iy >= S) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int ix = 2 * gx - 1 + kw;
        if (ix < 0 || ix >= S) continue;
        const int px = 2 * ox + kw;
        const float x = xs[ci * SU_PLANE + (2 * oy + kh) * SU_ROW + (px & 1) * SU_HALF + (px >> 1)];
        const float* wk = &wl[((ci * 3 + kh) * 3 + kw) * 16];
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[c] = fmaf(x, wk[c], acc[c]);
      }
    }
}

// the u8 stems' launch contract: whole tiles, dword-aligned rows, one grid row an image
inline bool stem_u8_fits(const void* crops, int ch, int B, int S) {
  return crops && !((uintptr_t)crops & 3) && (ch == 1 || ch == 3) && B > 0 && B <= 65535 && S >= 2 * SU_T &&
         S % (2 * SU_T) == 0;
}
