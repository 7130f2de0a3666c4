// Bottleneck tail + next conv1 for the wide block outputs (ResNet-50 layers 2 and 3, N1 = 512 /
// 1024), the streamed-weight sibling of btail.hip:
//
//     y[M][N1] = relu(A[M][K1] . W3^T + b3 (+ R))     conv3 1x1 + bn3 (+ identity) + relu   -> stored
//     z[M][N2] = relu(y . W1^T + b1)                  the NEXT block's conv1 1x1 + bn1 + relu -> stored
//
// W3 and W1 together are 256 KB (layer 2) or 1 MB (layer 3), so they cannot live in LDS as in
// btail.hip.  The shape is the fused FFN's (ffn.hip): a K1-wide input, an N1-wide hidden
// activation, an N2-wide output, the two weight matrices streamed in chunks of HC = 32 hidden
// channels -- except that here the hidden activation y also takes a residual and is stored.
//
// * One workgroup of 4 waves per row tile of 64 MB rows; a wave owns 16 MB rows: their A fragments
//   and the z^T accumulator (N2 x 16 MB, fp32) stay in registers for the tile's life.
// * Per chunk: W3's 32 rows, W1's 32 columns and the waves' own 16 MB x 32 pieces of R arrive in a
//   three-slot LDS ring by buffer_load ... lds, two chunks ahead.  Every load inside the loop is
//   such a DMA and every store a buffer store that dead rows aim past the buffer's end (dropped by
//   the range check), so every path issues the same memory instructions and the counted vmcnt
//   waits are exact (gemm_stream.hip explains why that matters).
// * First product in the C^T form MFMA(W3, A) with the chunk's W3 rows staged in ffn.hip's
//   w1_src_row order: lane (g, c16) owns row c16 and the 8 CONSECUTIVE channels 8g .. 8g+7 of the
//   chunk.  + b3 (+ R), ReLU, rounded to bf16 these 16 bytes are one store to y and, unchanged,
//   the B operand of the second product MFMA(W1, y) over K = 32 in W1's natural column order:
//   spe_btail_wide_perm is the identity.  z is exact up to the MFMA's internal summation order.
// * No persistence: with N2 = 128 two workgroups share a CU (208 registers, 77 KB of LDS), so
//   one tile's prologue and epilogue run beside the other's chunks; layer 3 at B = 64 has fewer
//   192-row tiles (226) than the chip has CUs.
#include "spe_common.h"
#include "spe_kernels.h"

#include <algorithm>
#include <cstdlib>

namespace {

typedef __attribute__((address_space(3))) void* lds_ptr_t;
constexpr int NT = 256, HC = 32, NST = 3;
constexpr int BAD = 0x7ffffff0;            // out-of-range buffer offset: loads give zero, stores are dropped
constexpr int N1MAX = 1024;

template <int N>
SPE_DEV void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// chunk channel held by LDS row r of the W3 stage (ffn.hip w1_src_row)
SPE_DEV int w3_src_row(int r) { return 8 * ((r & 15) >> 2) + 4 * (r >> 4) + (r & 3); }
// W1 stage: 16-byte piece c (chunk channels 8c .. 8c+7) of row n (ffn.hip w2_off)
SPE_DEV int w1_key(int n) { return (4 - ((n >> 2) & 3)) & 3; }
SPE_DEV int w1_off(int n, int c) { return n * 64 + ((c ^ w1_key(n)) << 4); }

// One chunk's DMA (buffer_load ... lds, 1 KB per wave instruction, linear LDS image, the swizzles
// applied on the source side): the buffer resources and the per-lane parts of the source
// addresses are fixed for the kernel's life, the chunk's offset is a scalar.  Rows past M aim
// past the residual's end and zero-fill.
template <int K1, int N2, int MB, bool HAS_R>
struct WideDma {
  static constexpr int KB1 = K1 * 2;
  static constexpr int W3_BYTES = HC * KB1, W1_BYTES = N2 * HC * 2;
  static constexpr int L3 = W3_BYTES / 1024 / 4, L1 = W1_BYTES / 1024 / 4;   // instructions per wave per chunk
  static constexpr int RPI = 1024 / KB1, LPR = KB1 / 16;   // W3 rows per instruction, lanes per row
  __amdgpu_buffer_rsrc_t r3, r1, rr;
  int vo3[L3], vo1[L1], vor[MB];
  SPE_DEV void init(const BtailArgs& a, int m0, int wid, int lane) {
    r3 = __builtin_amdgcn_make_buffer_rsrc((void*)a.w3, (short)0, a.n1 * a.ld3 * 2, 0x00020000);
    r1 = __builtin_amdgcn_make_buffer_rsrc((void*)a.w1, (short)0, N2 * a.ld1 * 2, 0x00020000);
    rr = __builtin_amdgcn_make_buffer_rsrc((void*)a.R, (short)0, HAS_R ? ((a.M - 1) * a.ldr + a.n1) * 2 : 0, 0x00020000);
#pragma unroll
    for (int i = 0; i < L3; ++i) {
      const int r = RPI * (wid * L3 + i) + lane / LPR, c = (lane % LPR) ^ (r & 15);
      vo3[i] = (w3_src_row(r) * a.ld3 + c * 8) * 2;
    }
#pragma unroll
    for (int i = 0; i < L1; ++i) {
      const int n = 16 * (wid * L1 + i) + (lane >> 2), c = (lane & 3) ^ w1_key(n);
      vo1[i] = (n * a.ld1 + c * 8) * 2;
    }
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const int m = m0 + 16 * mb + (lane & 15);
      vor[mb] = m < a.M ? (m * a.ldr + 8 * (lane >> 4)) * 2 : BAD;
    }
  }
  // chunk ch -> ring slot st: W3 rows (staged order), W1 columns, this wave's R pieces (lane-linear)
  SPE_DEV void issue(const BtailArgs& a, int ch, char* st, int wid) const {
#pragma unroll
    for (int i = 0; i < L3; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(r3, (lds_ptr_t)(st + (wid * L3 + i) * 1024), 16, vo3[i], ch * HC * a.ld3 * 2, 0, 0);
#pragma unroll
    for (int i = 0; i < L1; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(r1, (lds_ptr_t)(st + W3_BYTES + (wid * L1 + i) * 1024), 16, vo1[i], ch * HC * 2, 0, 0);
    if constexpr (HAS_R) {
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rr, (lds_ptr_t)(st + W3_BYTES + W1_BYTES + (wid * MB + mb) * 1024), 16, vor[mb],
                                                 ch * HC * 2, 0, 0);
    }
  }
};

// STORE_Y / RELU_Z are compile-time (the defaults are the layer-2 / layer-3 tails; the final tail of the
// stride-16 model below clears them): without STORE_Y the kernel holds no y store at all and never reads
// a.y, so in every instantiation every path still issues the same memory instructions and the counted
// waits count exactly what that instantiation issues.
template <int K1, int N2, int MB, bool HAS_R, bool STORE_Y = true, bool RELU_Z = true>
__global__ __launch_bounds__(NT, (N2 == 128 && MB <= 2) ? 2 : 1) void btail_wide_kernel(BtailArgs a) {
  constexpr int YST = STORE_Y ? MB : 0;      // y stores a chunk step issues
  constexpr int KB1 = K1 * 2, KF1 = K1 / 32, NB2 = N2 / 16;
  constexpr int W3_BYTES = HC * KB1, W1_BYTES = N2 * HC * 2, R_BYTES = HAS_R ? 4 * MB * 1024 : 0;
  constexpr int STAGE = W3_BYTES + W1_BYTES + R_BYTES;
  constexpr int L3 = W3_BYTES / 1024 / 4, L1 = W1_BYTES / 1024 / 4;   // DMA instructions per wave per chunk
  constexpr int LOADS = L3 + L1 + (HAS_R ? MB : 0);
  // one LDS array (a second __shared__ object beside in-flight LDS DMA can make the compiler drain
  // vmcnt before LDS reads): [NST stages][b3][b1]
  __shared__ __attribute__((aligned(1024))) char lds[NST * STAGE + (N1MAX + N2) * 4];
  float* sb3 = reinterpret_cast<float*>(lds + NST * STAGE);
  float* sb1 = sb3 + N1MAX;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  const int m0 = blockIdx.x * 64 * MB + wid * 16 * MB;
  const int nch = a.n1 / HC;
  for (int i = tid; i < a.n1; i += NT) sb3[i] = a.b3[i];
  for (int i = tid; i < N2; i += NT) sb1[i] = a.b1[i];

  // A rows of this wave as B fragments: xf[mb][ks] = A[m0 + 16mb + c16][32ks + 8g .. +7]
  bf16x8 xf[MB][KF1];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = m0 + 16 * mb + c16;
    const bf16* xr = (const bf16*)a.A + (size_t)(m < a.M ? m : 0) * a.lda;
#pragma unroll
    for (int ks = 0; ks < KF1; ++ks)
      xf[mb][ks] = __builtin_bit_cast(bf16x8, m < a.M ? ld16(xr + 32 * ks + 8 * g) : u32x4{0, 0, 0, 0});
  }
  f32x4 acc[NB2][MB];
#pragma unroll
  for (int nb = 0; nb < NB2; ++nb)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[nb][mb] = f32x4{0, 0, 0, 0};

  // (without STORE_Y: an empty range that nothing stores to)
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(
      STORE_Y ? a.y : nullptr, (short)0, STORE_Y ? ((a.M - 1) * a.ldy + a.n1) * 2 : 0, 0x00020000);
  int voy[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = m0 + 16 * mb + c16;
    voy[mb] = STORE_Y && m < a.M ? (m * a.ldy + 8 * g) * 2 : BAD;
  }
  WideDma<K1, N2, MB, HAS_R> dma;
  dma.init(a, m0, wid, lane);

  // A (and b3) retired before the DMA starts: vmcnt is in order, and with a load of A pending at
  // the loop entry the compiler's merged wait state would drain every in-flight chunk (ffn.hip)
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int ks = 0; ks < KF1; ++ks) asm volatile("" ::"v"(xf[mb][ks]));
  wait_vmcnt<0>();
  dma.issue(a, 0, lds, wid);
  dma.issue(a, 1, lds + STAGE, wid);                          // (nch >= 16)

  int slot = 0;
  for (int ch = 0; ch < nch; ++ch) {
    // Issue order: DMA(ch) [step ch-2], y stores(ch-2), DMA(ch+1), y stores(ch-1), this wait.  Chunk ch
    // and the stores of step ch-2 retire; chunk ch+1 and the MB stores of step ch-1 may stay in flight
    // (without STORE_Y there are no stores: YST = 0 and only chunk ch+1 stays in flight).
    if (ch == 0) wait_vmcnt<LOADS>();
    else if (ch + 1 < nch) wait_vmcnt<LOADS + YST>();
    else wait_vmcnt<YST>();
    // raw barrier (__syncthreads' fence would drain the chunk in flight): every wave's part of chunk
    // ch is visible, and the slot of chunk ch+2 -- read in step ch-1 -- is free
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const int slot2 = slot == 0 ? NST - 1 : slot - 1;       // (ch + 2) % NST
    const char* st = lds + slot * STAGE;
    slot = slot == NST - 1 ? 0 : slot + 1;
    u32x4 wa[KF1][2], wb[NB2], rv[HAS_R ? MB : 1];
#pragma unroll
    for (int ks = 0; ks < KF1; ++ks)
#pragma unroll
      for (int jb = 0; jb < 2; ++jb) {
        const int r = 16 * jb + c16;
        wa[ks][jb] = ld16(st + r * KB1 + (((4 * ks + g) ^ (r & 15)) << 4));
      }
    if constexpr (HAS_R) {
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) rv[mb] = ld16(st + W3_BYTES + W1_BYTES + (wid * MB + mb) * 1024 + lane * 16);
    }
#pragma unroll
    for (int nb = 0; nb < NB2; ++nb) wb[nb] = ld16(st + W3_BYTES + w1_off(16 * nb + c16, g));
    // the next DMA goes out after this chunk's LDS reads: issued before them, the compiler (which
    // cannot tell the DMA's slot from the read's) would drain it first
    if (ch + 2 < nch) dma.issue(a, ch + 2, lds + slot2 * STAGE, wid);
    __builtin_amdgcn_sched_barrier(0);
    // ---- y^T chunk [32 j][16 MB m] = W3[j] . A[m]: h[jb][mb][r] <-> chunk channel 8g + 4jb + r
    f32x4 h[2][MB];
#pragma unroll
    for (int jb = 0; jb < 2; ++jb)
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) h[jb][mb] = f32x4{0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < KF1; ++ks)
#pragma unroll
      for (int jb = 0; jb < 2; ++jb) {
        const bf16x8 w = __builtin_bit_cast(bf16x8, wa[ks][jb]);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
          h[jb][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, xf[mb][ks], h[jb][mb], 0, 0, 0);
      }
    // ---- + b3 (+ R), ReLU, bf16: the 16 bytes stored to y are the second product's B operand
    const f32x4 b3a = *reinterpret_cast<const f32x4*>(sb3 + ch * HC + 8 * g);
    const f32x4 b3b = *reinterpret_cast<const f32x4*>(sb3 + ch * HC + 8 * g + 4);
    bf16x8 yb[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      float v[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] = h[0][mb][r] + b3a[r];
        v[4 + r] = h[1][mb][r] + b3b[r];
      }
      if constexpr (HAS_R) {
        float rf[8];
        unpack16<bf16>(rv[mb], rf);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += rf[e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
      const u32x4 yw = pack16<bf16>(v);
      if constexpr (STORE_Y) __builtin_amdgcn_raw_buffer_store_b128(yw, ry, voy[mb], ch * HC * 2, 0);
      yb[mb] = __builtin_bit_cast(bf16x8, yw);
    }
    // ---- z^T[n][m] += W1[n][chunk 8g .. 8g+7] . y^T[8g .. 8g+7][m]
#pragma unroll
    for (int nb = 0; nb < NB2; ++nb) {
      const bf16x8 w = __builtin_bit_cast(bf16x8, wb[nb]);
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
        acc[nb][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, yb[mb], acc[nb][mb], 0, 0, 0);
    }
  }

  // ---- z = relu(acc + b1), or acc + b1 without RELU_Z (b1 from LDS: loads from memory would be ordered against the z stores
  // one by one): the lane holds, for row m0 + 16mb + c16, columns 16nb + 4g + r
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = m0 + 16 * mb + c16;
    if (m >= a.M) continue;
    bf16* zr = (bf16*)a.z + (size_t)m * a.ldz;
#pragma unroll
    for (int nb = 0; nb < NB2; ++nb) {
      const int n = 16 * nb + 4 * g;
      const f32x4 bv = *reinterpret_cast<const f32x4*>(sb1 + n);
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = RELU_Z ? fmaxf(acc[nb][mb][r] + bv[r], 0.f) : acc[nb][mb][r] + bv[r];
      st8(zr + n, u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])});
    }
  }
}

// The final tail of the stride-16 model (K1 = 256, N1 = 1024, N2 = 256, 192-row tiles): the last bottleneck's
// conv3 + identity + relu with input_proj as the second product -- z without the ReLU, and y, which nobody
// else reads, not stored.
// (explicit instantiations: left implicit, the host compiler emits the launch stubs of only some of them)
#define SPE_BTAIL_WIDE_INST(R, Y, Z) template __global__ void btail_wide_kernel<256, 256, 3, R, Y, Z>(BtailArgs);
SPE_BTAIL_WIDE_INST(false, false, false) SPE_BTAIL_WIDE_INST(false, false, true) SPE_BTAIL_WIDE_INST(false, true, false)
SPE_BTAIL_WIDE_INST(false, true, true) SPE_BTAIL_WIDE_INST(true, false, false) SPE_BTAIL_WIDE_INST(true, false, true)
SPE_BTAIL_WIDE_INST(true, true, false) SPE_BTAIL_WIDE_INST(true, true, true)
#undef SPE_BTAIL_WIDE_INST

template <bool HAS_R, bool STORE_Y, bool RELU_Z>
int launch_proj(const BtailArgs& a, hipStream_t s) {
  const int tiles = (a.M + 191) / 192;
  hipLaunchKernelGGL((btail_wide_kernel<256, 256, 3, HAS_R, STORE_Y, RELU_Z>), dim3(tiles), dim3(NT), 0, s, a);
  return (int)hipGetLastError();
}

template <int K1, int N2, int MB>
int launch(const BtailArgs& a, hipStream_t s) {
  const int tiles = (a.M + 64 * MB - 1) / (64 * MB);
  if (a.R) hipLaunchKernelGGL((btail_wide_kernel<K1, N2, MB, true>), dim3(tiles), dim3(NT), 0, s, a);
  else hipLaunchKernelGGL((btail_wide_kernel<K1, N2, MB, false>), dim3(tiles), dim3(NT), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace

// K order of the second product's weights: stored column k holds channel perm(k).  The first
// product's staged row order leaves each lane with 8 consecutive channels (header above), so the
// wide kernel reads W1 in its natural order.
int spe_btail_wide_perm(int n1, int k) { return k >= 0 && k < n1 ? k : -1; }

bool spe_btail_wide_enabled() {
  static const int on = spe_env_int("SPE_BTAIL_WIDE", 1);
  return on != 0;
}

namespace {
// rows per workgroup tile: 64 MB
int tile_rows(const BtailArgs& a) { return a.n1 == 1024 ? 192 : 128; }
}  // namespace

int spe_btail_wide_tiles(const BtailArgs& a) { return (a.M + tile_rows(a) - 1) / tile_rows(a); }

// y may be null for the final form (spe_launch_btail_wide_proj), which stores none
static bool strides_served(const BtailArgs& a) {
  const int ldy = a.y ? a.ldy : a.n1;
  if (a.lda % 8 || ldy % 8 || a.ldz % 4 || (a.R && a.ldr % 8) || a.lda < a.k1 || ldy < a.n1 || a.ldz < a.n2 ||
      (a.R && a.ldr < a.n1) || a.ld3 < a.k1 || a.ld1 < a.n1 || a.ld3 % 8 || a.ld1 % 8)
    return false;
  // 32-bit buffer offsets
  return (double)a.M * std::max(a.y ? a.ldy : 0, a.R ? a.ldr : 0) * 2 < 2147483648.0;
}

// Off by default: in the measured B = 64, 448^2 step the fused launch was not faster than its two GEMMs
// (backbone stage 3.605 against 3.600 ms, profiles/backbone_s16_vs_s8.json)
bool spe_btail_wide_proj_enabled() {
  static const int on = spe_env_int("SPE_BTAIL_PROJ", 0);
  return on != 0;
}

bool spe_btail_wide_proj_serves(const BtailArgs& a) {
  if (!spe_btail_wide_enabled() || !a.A || !a.w3 || !a.b3 || !a.w1 || !a.b1 || !a.z) return false;
  return strides_served(a) && a.k1 == 256 && a.n1 == 1024 && a.n2 == 256;
}

// 1 = not a problem for this kernel
int spe_launch_btail_wide_proj(const BtailArgs& a, bool relu_z, hipStream_t s) {
  if (a.M <= 0) return 0;
  if (!spe_btail_wide_proj_serves(a)) return 1;
  if (a.y && relu_z) return spe_launch_btail_wide(a, s);
  const int sel = (a.R ? 4 : 0) | (a.y ? 2 : 0) | (relu_z ? 1 : 0);
  switch (sel) {
    case 0: return launch_proj<false, false, false>(a, s);
    case 1: return launch_proj<false, false, true>(a, s);
    case 2: return launch_proj<false, true, false>(a, s);
    case 4: return launch_proj<true, false, false>(a, s);
    case 5: return launch_proj<true, false, true>(a, s);
    default: return launch_proj<true, true, false>(a, s);
  }
}

bool spe_btail_wide_serves(const BtailArgs& a) {
  if (!spe_btail_wide_enabled() || !a.y) return false;
  if (a.lda % 8 || a.ldy % 8 || a.ldz % 4 || (a.R && a.ldr % 8) || a.lda < a.k1 || a.ldy < a.n1 || a.ldz < a.n2 ||
      (a.R && a.ldr < a.n1) || a.ld3 < a.k1 || a.ld1 < a.n1 || a.ld3 % 8 || a.ld1 % 8)
    return false;
  // 32-bit buffer offsets
  if ((double)a.M * std::max(a.ldy, a.R ? a.ldr : 0) * 2 >= 2147483648.0) return false;
  return (a.k1 == 128 && a.n1 == 512 && (a.n2 == 128 || a.n2 == 256)) || (a.k1 == 256 && a.n1 == 1024 && a.n2 == 256);
}

// 1 = not a problem for this kernel
int spe_launch_btail_wide(const BtailArgs& a, hipStream_t s) {
  if (a.M <= 0) return 0;
  if (!spe_btail_wide_serves(a)) return 1;
  if (a.n1 == 1024) return launch<256, 256, 3>(a, s);
  if (a.n2 == 128) return launch<128, 128, 2>(a, s);
  return launch<128, 256, 2>(a, s);
}
