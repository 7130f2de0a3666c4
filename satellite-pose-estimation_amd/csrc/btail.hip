// Bottleneck tail + next conv1 in one streaming pass (ResNet-50 layer 1, REV/models/backbone.py
// :114-125, torchvision Bottleneck):
//
//     y = relu(A . W3^T + b3 (+ R))          conv3 1x1 + bn3 (+ identity) + relu   -> stored
//     z = relu(y . W1^T + b1)                the NEXT block's conv1 1x1 + bn1 + relu -> stored
//
// The separate launches read y back from HBM right after writing it (354 MB per 64-image layer-1
// boundary); here y goes to HBM once (it is the next block's residual) and feeds the second
// product from registers.  y is N1 = 256 channels, the conv3 input K1 = 64 (or 128: block 0's
// [conv2 output | max-pool output] concatenation, registry.cpp c3ds), the next conv1 N2 = 64
// (layer 1) or 128 (layer 2 block 0).
//
// * Persistent workgroup of 8 waves per CU; W3 and W1 live in LDS for the kernel's life
//   (XOR-swizzled 16-byte chunks, conflict-free fragment reads).  Each wave streams 16-row
//   tiles: A and R of the next tile are loaded before the current one is multiplied.
// * First product in the C^T form MFMA(W3, A): a lane owns row m = fr and channels
//   16 j + 4 fg + r of y -- the store layout (8-byte row pieces) and, packed to bf16, the
//   operand of the second product without any data movement: for K-chunk kc the lane's 8
//   elements are channels 32 kc + 4 fg + {0..3} and 32 kc + 16 + 4 fg + {0..3}.  W1 is stored
//   with its columns permuted the same way (btail_perm, registry.cpp), so MFMA(W1p, y) pairs
//   them correctly; z is exact up to the MFMA's internal summation order.
// * ROWS (BtailArgs::rows, the default): the LDS images of W3 and W1 take their rows in
//   spe_btail_row_perm order, so the fragment pair (2i, 2i+1) leaves a lane the 8 CONSECUTIVE channels
//   32 i + 8 sg .. + 7, sg = fg with its two bits swapped: R, y and z move as 16-byte row pieces (8
//   instructions per 512-byte row instead of 16, 64 contiguous bytes per row and instruction).  For the
//   second product one v_permlane16_swap per register pair trades the piece's upper half in lane groups
//   0 / 2 for the lower half in groups 1 / 3, which leaves every lane group with exactly the channels
//   4 fg + {0..3} and 16 + 4 fg + {0..3} it has without ROWS: W1p and every MFMA K slot stay as they
//   were, so y and z are bit-identical.  (With the plain order 8 fg and W1 in natural column order z
//   was NOT: the MFMA's internal sum depends on the slot, 1 of 8256 and 4 of 33408 elements differed.)
// * YC (the layer-1 -> layer-2 tail): y is read only by the next block's stride-2 downsample, so only
//   the pixels with even h and even w are stored, densely, as [B][H/2][W/2][N1].
#include "spe_common.h"
#include "spe_kernels.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace {

typedef __attribute__((address_space(3))) void* lds_ptr_t;
constexpr int N1 = 256, NT = 512, NW = 8;

template <int K1, int N2, bool HAS_R, bool ROWS, bool YC>
__global__ __launch_bounds__(NT, 1) void btail_kernel(BtailArgs a, int row_tiles) {
  constexpr int KB1 = K1 * 2, KF1 = K1 / 32;          // W3 row bytes, K fragments of the first product
  constexpr int KB2 = N1 * 2;                          // W1 row bytes (K2 = N1)
  constexpr int J1 = N1 / 16, J2 = N2 / 16;            // column fragments
  __shared__ __attribute__((aligned(1024))) char w3s[N1 * KB1];
  __shared__ __attribute__((aligned(1024))) char w1s[N2 * KB2];
  __shared__ __attribute__((aligned(16))) float sb3[N1], sb1[N2];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fg = lane >> 4, fr = lane & 15;
  const int sg = ((fg & 1) << 1) | (fg >> 1);          // ROWS: the lane's 16-byte piece within 64 bytes
  // ---- weights -> LDS.  Row n, 16-byte chunk c at n*KB + (c ^ (n & wkey_mask(KB)))*16; one
  // direct-to-LDS wave instruction fills 1 KB linearly, the swizzle applied on the source.
  {
    constexpr int INS3 = N1 * KB1 / 1024, INS1 = N2 * KB2 / 1024;
    for (int q = wid; q < INS3 + INS1; q += NW) {
      const bool first = q < INS3;
      const int qq = first ? q : q - INS3, KB = first ? KB1 : KB2;
      const int o = qq * 1024 + lane * 16;
      const int n = o / KB, within = o - n * KB;
      const int chunk = (within >> 4) ^ (n & wkey_mask(KB));
      const int ns = ROWS ? spe_btail_row_perm(n) : n;     // the weight row that LDS row n holds
      const char* src = first ? (const char*)a.w3 + (size_t)ns * a.ld3 * 2 + chunk * 16
                              : (const char*)a.w1 + (size_t)ns * a.ld1 * 2 + chunk * 16;
      __builtin_amdgcn_global_load_lds((const void*)src, (lds_ptr_t)((first ? w3s : w1s) + qq * 1024), 16, 0, 0);
    }
    for (int i = tid; i < N1; i += NT) sb3[i] = a.b3[i];
    for (int i = tid; i < N2; i += NT) sb1[i] = a.b1[i];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  auto w_addr = [](int n, int chunk, int KB) { return wkey_addr(n, chunk, KB); };

  auto load_a = [&](int t, u32x4 (&x)[KF1]) {
    t = t < row_tiles ? t : row_tiles - 1;
    int m = t * 16 + fr;
    m = m < a.M ? m : a.M - 1;
    const char* p = (const char*)a.A + (size_t)m * a.lda * 2 + fg * 16;
#pragma unroll
    for (int kf = 0; kf < KF1; ++kf) x[kf] = ld16(p + kf * 64);
  };
  // row pieces of R, y and z: 8 bytes (channels 16 j + 4 fg ..) or, with ROWS, 16 (32 i + 8 fg ..)
  using piece_t = std::conditional_t<ROWS, u32x4, u32x2>;
  constexpr int P1 = ROWS ? J1 / 2 : J1, PR = HAS_R ? P1 : 1;
  auto load_r = [&](int t, piece_t (&r)[PR]) {
    if constexpr (HAS_R) {
      t = t < row_tiles ? t : row_tiles - 1;
      int m = t * 16 + fr;
      m = m < a.M ? m : a.M - 1;
      if constexpr (ROWS) {
        const char* p = (const char*)a.R + ((size_t)m * a.ldr + 8 * sg) * 2;
#pragma unroll
        for (int i = 0; i < P1; ++i) r[i] = ld16(p + i * 64);
      } else {
        const char* p = (const char*)a.R + ((size_t)m * a.ldr + 4 * fg) * 2;
#pragma unroll
        for (int j = 0; j < J1; ++j) r[j] = ld8(p + j * 32);
      }
    }
  };

  const int G = gridDim.x;
  const int stride = G * NW;
  const int t0 = xcd_remap(blockIdx.x, G) * NW + wid;
  if (t0 >= row_tiles) return;
  auto tile = [&](int t, const u32x4 (&ab)[KF1], const piece_t (&rb)[PR]) {
    // (a compiler-only fence: the weight fragments are loop-invariant LDS reads, and hoisting
    // them out of the tile loop would pin 256 registers)
    asm volatile("" ::: "memory");
    f32x4 acc[J1];
#pragma unroll
    for (int j = 0; j < J1; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kf = 0; kf < KF1; ++kf) {
      const bf16x8 av = __builtin_bit_cast(bf16x8, ab[kf]);
#pragma unroll
      for (int j = 0; j < J1; ++j) {
        const bf16x8 w = __builtin_bit_cast(bf16x8, ld16(w3s + w_addr(16 * j + fr, 4 * kf + fg, KB1)));
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, av, acc[j], 0, 0, 0);
      }
    }
    // ---- y = relu(acc + b3 (+ R)): store, and pack as the second product's operand
    const int m = t * 16 + fr;
    const bool ok = m < a.M;
    // YC: the row's pixel, decoded once per tile; the even-h even-w pixels go to dense rows
    int my = m;
    bool oky = ok;
    if constexpr (YC) {
      const unsigned hw = (unsigned)a.H * a.W, b = (unsigned)m / hw, rem = (unsigned)m - b * hw;
      const unsigned h = rem / (unsigned)a.W, w = rem - h * a.W;
      oky = ok && !((h | w) & 1);
      my = (int)((b * (a.H >> 1) + (h >> 1)) * (a.W >> 1) + (w >> 1));
    }
    piece_t yw[P1];
    if constexpr (ROWS) {
      char* yp = (char*)a.y + ((size_t)my * a.ldy + 8 * sg) * 2;
#pragma unroll
      for (int i = 0; i < P1; ++i) {
        const f32x4 ba = *reinterpret_cast<const f32x4*>(sb3 + 32 * i + 8 * sg);
        const f32x4 bb = *reinterpret_cast<const f32x4*>(sb3 + 32 * i + 8 * sg + 4);
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = acc[2 * i][e] + ba[e];
          v[4 + e] = acc[2 * i + 1][e] + bb[e];
        }
        if constexpr (HAS_R) {
          float rf[8];
          unpack16<bf16>(rb[i], rf);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += rf[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
        yw[i] = pack16<bf16>(v);
        if (oky) st16(yp + i * 64, yw[i]);
      }
    } else {
      char* yp = (char*)a.y + ((size_t)my * a.ldy + 4 * fg) * 2;
#pragma unroll
      for (int j = 0; j < J1; ++j) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(sb3 + 16 * j + 4 * fg);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[j][e] + bv[e];
        if constexpr (HAS_R) {
          v[0] += __uint_as_float(rb[j].x << 16);
          v[1] += __uint_as_float(rb[j].x & 0xffff0000u);
          v[2] += __uint_as_float(rb[j].y << 16);
          v[3] += __uint_as_float(rb[j].y & 0xffff0000u);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        yw[j] = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
        if (oky) st8(yp + j * 32, yw[j]);
      }
    }
    // ---- z = relu(y . W1^T + b1), K-chunk kc = column fragments 2kc, 2kc+1 of y
    f32x4 acc2[J2];
#pragma unroll
    for (int j = 0; j < J2; ++j) acc2[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kc = 0; kc < N1 / 32; ++kc) {
      bf16x8 yv;
      if constexpr (ROWS) {
        // lane groups (0, 1) hold channels (0-7, 16-23) of the chunk, (2, 3) hold (8-15, 24-31): the swap
        // (odd 16-lane rows of the first operand <-> even rows of the second) gives group g 4g.., 16 + 4g..
        const u32x2 s0 = __builtin_amdgcn_permlane16_swap(yw[kc].x, yw[kc].z, false, false);
        const u32x2 s1 = __builtin_amdgcn_permlane16_swap(yw[kc].y, yw[kc].w, false, false);
        yv = __builtin_bit_cast(bf16x8, u32x4{s0.x, s1.x, s0.y, s1.y});
      } else yv = __builtin_bit_cast(bf16x8, u32x4{yw[2 * kc].x, yw[2 * kc].y, yw[2 * kc + 1].x, yw[2 * kc + 1].y});
#pragma unroll
      for (int j = 0; j < J2; ++j) {
        const bf16x8 w = __builtin_bit_cast(bf16x8, ld16(w1s + w_addr(16 * j + fr, 4 * kc + fg, KB2)));
        acc2[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, yv, acc2[j], 0, 0, 0);
      }
    }
    asm volatile("" ::: "memory");
    if constexpr (ROWS) {
      char* zp = (char*)a.z + ((size_t)m * a.ldz + 8 * sg) * 2;
#pragma unroll
      for (int i = 0; i < J2 / 2; ++i) {
        const f32x4 ba = *reinterpret_cast<const f32x4*>(sb1 + 32 * i + 8 * sg);
        const f32x4 bb = *reinterpret_cast<const f32x4*>(sb1 + 32 * i + 8 * sg + 4);
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = fmaxf(acc2[2 * i][e] + ba[e], 0.f);
          v[4 + e] = fmaxf(acc2[2 * i + 1][e] + bb[e], 0.f);
        }
        if (ok) st16(zp + i * 64, pack16<bf16>(v));
      }
    } else {
      char* zp = (char*)a.z + ((size_t)m * a.ldz + 4 * fg) * 2;
#pragma unroll
      for (int j = 0; j < J2; ++j) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(sb1 + 16 * j + 4 * fg);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(acc2[j][e] + bv[e], 0.f);
        if (ok) st8(zp + j * 32, u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])});
      }
    }
  };

  // two operand sets in rotation (unrolled by two: register arrays are never indexed at run
  // time): the next tile's A and R are in flight while the current tile is multiplied
  u32x4 a0[KF1], a1[KF1];
  piece_t r0[PR], r1[PR];
  load_a(t0, a0);
  load_r(t0, r0);
  for (int t = t0;;) {
    load_a(t + stride, a1);
    load_r(t + stride, r1);
    tile(t, a0, r0);
    t += stride;
    if (t >= row_tiles) break;
    load_a(t + stride, a0);
    load_r(t + stride, r0);
    tile(t, a1, r1);
    t += stride;
    if (t >= row_tiles) break;
  }
}

template <int K1, int N2, bool HAS_R, bool ROWS, bool YC = false>
int launch(const BtailArgs& a, hipStream_t s) {
  const int row_tiles = (a.M + 15) / 16;
  const int G = spe_cu_count();
  hipLaunchKernelGGL((btail_kernel<K1, N2, HAS_R, ROWS, YC>), dim3(G), dim3(NT), 0, s, a, row_tiles);
  return (int)hipGetLastError();
}

template <bool ROWS>
int launch_shape(const BtailArgs& a, bool yc, hipStream_t s) {
  if (a.k1 == 64 && a.n2 == 64 && a.R) return launch<64, 64, true, ROWS>(a, s);
  if (a.k1 == 64 && a.n2 == 128 && a.R) return yc ? launch<64, 128, true, ROWS, true>(a, s) : launch<64, 128, true, ROWS>(a, s);
  if (a.k1 == 128 && a.n2 == 64 && !a.R) return launch<128, 64, false, ROWS>(a, s);
  return 1;
}

}  // namespace

// K-order permutation of the second product's weights (header above), the same for both row-piece forms:
// stored column 32 kc + 8 g + e holds channel 32 kc + (e < 4 ? 4 g + e : 16 + 4 g + e - 4).
int spe_btail_perm(int k) {
  const int kc = k >> 5, g = (k >> 3) & 3, e = k & 7;
  return 32 * kc + (e < 4 ? 4 * g + e : 16 + 4 * g + e - 4);
}

bool spe_btail_enabled() {
  static const int on = spe_env_int("SPE_BTAIL", 1);
  return on != 0;
}

// SPE_BTAIL_ROWS=0: the 8-byte row pieces; SPE_BTAIL_YCOMPACT=0: every tail stores its whole y (A/B
// knobs).  Not cached: a model reads them once, when it is finalized, and keeps what it read.
bool spe_btail_rows_enabled() { return spe_env_int("SPE_BTAIL_ROWS", 1) != 0; }
bool spe_btail_ycompact_enabled() { return spe_env_int("SPE_BTAIL_YCOMPACT", 1) != 0; }

// the compact y store applies: the one instantiation that has it, rows = whole images of even edges
bool spe_btail_ycompact_serves(const BtailArgs& a) {
  return a.ycompact && a.H > 0 && a.W > 0 && a.H % 2 == 0 && a.W % 2 == 0 && a.M % (a.H * a.W) == 0 && a.k1 == 64 &&
         a.n2 == 128 && a.R;
}

// 1 = not a problem for this kernel
int spe_launch_btail(const BtailArgs& a, hipStream_t s) {
  if (a.M <= 0) return 0;
  const int al = a.rows ? 8 : 4;             // 16-byte pieces need 16-byte aligned rows
  if (a.lda % 8 || a.ldy % al || a.ldz % al || (a.R && a.ldr % al) || a.ld3 < a.k1 || a.ld1 < a.n1) return 1;
  if (a.n1 != N1) return 1;
  const bool yc = spe_btail_ycompact_serves(a);
  return a.rows ? launch_shape<true>(a, yc, s) : launch_shape<false>(a, yc, s);
}
