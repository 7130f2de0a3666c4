// GroupNorm(32, C) over the backbone's NHWC activation rows [B*H*W][ld] (REV/models/backbone.py:168-170,
// MyGroupNorm = nn.GroupNorm(32, C), eps 1e-5), optionally followed by a residual add and a ReLU
// (torchvision Bottleneck.forward: out = relu(bn3(conv3) + identity)).  bf16 and fp32 storage.
//
// Two launches per norm layer, no atomics, a fixed summation order (the same input gives the same bits):
//
//   norm.gn.stats  grid (tiles, B): the pixels of an image are cut into tiles of GN_TILE_ELEMS / C pixels and one
//                  work-group reduces every group of its tile to a Welford triple (count, mean, M2) in
//                  part[b][tile][32][3].  A thread owns one 16-byte column of the rows and walks the tile's pixels, so a
//                  wave reads whole rows (or 64 consecutive 16-byte pieces of one): each vector gives, per group it
//                  touches, its own mean and squares about that mean (exact two-pass, in registers), merged into the
//                  thread's running triple (Chan et al.); lanes that share a group merge by xor shuffles, the four waves
//                  through LDS.  Nothing is ever squared before its mean is subtracted, so a large common offset
//                  (x = 100 + N(0, 1)) costs no digits -- the one-pass E[x^2] - E[x]^2 loses them all in fp32.
//   norm.gn.apply  the same grid: every work-group first re-merges its image's `tiles` triples per group (8 threads a
//                  group over the tiles, a shuffle tree, fixed order; biased variance), then streams its tile:
//                  y = (x - mean) * (rstd * gamma[c]) + beta[c] (+ residual) (ReLU), 16 bytes in and out per lane.
//                  x, residual and y may alias each other: an element is read and written by the one thread that owns it.
//
// C / 32 (channels per group) is 2, 4, 8, 16 or 32; a 16-byte vector (8 bf16 / 4 fp32) then lies inside one group or
// covers NG = 2 or 4 whole groups, the kernels' template parameter.
#include "spe_common.h"
#include "spe_kernels.h"

namespace {

constexpr int GN_GROUPS = 32;
constexpr int GN_THREADS = 256;
constexpr int GN_TILE_ELEMS = 16384;     // elements of one stats tile: GN_TILE_ELEMS / C pixels of all C channels
constexpr float GN_EPS = 1e-5f;

struct Wf { float n, mean, m2; };

// Chan's pairwise update; either side may be empty (n = 0)
SPE_DEV Wf wf_merge(Wf a, Wf b) {
  const float n = a.n + b.n;
  const float r = n > 0.f ? b.n / n : 0.f;
  const float d = b.mean - a.mean;
  return Wf{n, a.mean + d * r, a.m2 + b.m2 + d * d * a.n * r};
}
SPE_DEV Wf wf_shfl_xor(Wf a, int o) {
  return Wf{__shfl_xor(a.n, o, 64), __shfl_xor(a.mean, o, 64), __shfl_xor(a.m2, o, 64)};
}

template <typename T, int NG>
__global__ __launch_bounds__(GN_THREADS) void gn_stats_kernel(const T* __restrict__ x, int ldx, float* __restrict__ part,
                                                              int HW, int C, int PT, int tiles) {
  constexpr int V = Chunk<T>::CE, E = V / NG;      // E elements of a vector per group
  __shared__ float red[GN_THREADS / 64][GN_GROUPS][3];
  const int tile = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int cpg = C / GN_GROUPS, VR = C / V, RPB = GN_THREADS / VR;   // 16-byte columns of a row, rows per pass
  const int vc = t % VR, pr = t / VR;
  const int p1 = min(HW, (tile + 1) * PT);
  const T* xb = x + (size_t)b * HW * ldx + vc * V;
  float mean[NG], m2[NG];
#pragma unroll
  for (int j = 0; j < NG; ++j) mean[j] = m2[j] = 0.f;
  int it = 0;
  for (int p = tile * PT + pr; p < p1; p += RPB, ++it) {
    float f[V];
    unpack16<T>(ld16(xb + (size_t)p * ldx), f);
    // every running triple of this thread holds it * E elements: b.n / n = 1 / (it + 1), a.n b.n / n = it E / (it + 1)
    const float r = 1.f / (float)(it + 1), wgt = (float)(it * E) * r;
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < E; ++i) s += f[j * E + i];
      const float cm = s * (1.f / E);
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < E; ++i) { const float d = f[j * E + i] - cm; q += d * d; }
      const float d = cm - mean[j];
      mean[j] += d * r;
      m2[j] += q + d * d * wgt;
    }
  }
  Wf w[NG];
#pragma unroll
  for (int j = 0; j < NG; ++j) w[j] = Wf{(float)(it * E), mean[j], m2[j]};
  // lanes of a wave that hold the same group: the cpg / V neighbouring columns of a wide group, and the same column
  // of the wave's other rows (VR < 64)
  const int CG = cpg > V ? cpg / V : 1;
  for (int o = 1; o < CG; o <<= 1)
#pragma unroll
    for (int j = 0; j < NG; ++j) w[j] = wf_merge(w[j], wf_shfl_xor(w[j], o));
  for (int o = VR; o < 64; o <<= 1)
#pragma unroll
    for (int j = 0; j < NG; ++j) w[j] = wf_merge(w[j], wf_shfl_xor(w[j], o));
  if (t < (GN_THREADS / 64) * GN_GROUPS) red[t / GN_GROUPS][t % GN_GROUPS][0] = 0.f;   // groups a wave does not cover stay empty
  __syncthreads();
  const int lane = t & 63;
  if ((VR >= 64 || lane < VR) && vc % CG == 0) {
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      float* d = red[t >> 6][(vc * V + j * E) / cpg];
      d[0] = w[j].n; d[1] = w[j].mean; d[2] = w[j].m2;
    }
  }
  __syncthreads();
  if (t < GN_GROUPS) {
    Wf a{0.f, 0.f, 0.f};
#pragma unroll
    for (int wv = 0; wv < GN_THREADS / 64; ++wv)
      if (red[wv][t][0] > 0.f) a = wf_merge(a, Wf{red[wv][t][0], red[wv][t][1], red[wv][t][2]});
    float* d = part + (((size_t)b * tiles + tile) * GN_GROUPS + t) * 3;
    d[0] = a.n; d[1] = a.mean; d[2] = a.m2;
  }
}

template <typename T, int NG>
__global__ __launch_bounds__(GN_THREADS) void gn_apply_kernel(const T* x, int ldx, const T* res, int ldr,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, T* y, int ldy,
                                                              const float* __restrict__ part, int HW, int C, int PT,
                                                              int tiles, int relu) {
  constexpr int V = Chunk<T>::CE, E = V / NG;
  __shared__ float st[GN_GROUPS][2];               // mean, rstd
  const int tile = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  {
    const int g = t >> 3, k = t & 7;
    const float* pb = part + (size_t)b * tiles * GN_GROUPS * 3;
    Wf a{0.f, 0.f, 0.f};
    for (int tl = k; tl < tiles; tl += 8) {
      const float* q = pb + ((size_t)tl * GN_GROUPS + g) * 3;
      a = wf_merge(a, Wf{q[0], q[1], q[2]});
    }
    for (int o = 1; o < 8; o <<= 1) a = wf_merge(a, wf_shfl_xor(a, o));
    if (k == 0) {
      st[g][0] = a.mean;
      st[g][1] = 1.f / sqrtf(a.m2 / a.n + GN_EPS);
    }
  }
  __syncthreads();
  const int cpg = C / GN_GROUPS, VR = C / V, RPB = GN_THREADS / VR;
  const int vc = t % VR, pr = t / VR;
  float mu[V], sc[V], sh[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int c = vc * V + i, g = (vc * V + (i / E) * E) / cpg;
    mu[i] = st[g][0];
    sc[i] = st[g][1] * gamma[c];
    sh[i] = beta[c];
  }
  const int p1 = min(HW, (tile + 1) * PT);
  const size_t row0 = (size_t)b * HW;
  for (int p = tile * PT + pr; p < p1; p += RPB) {
    float f[V], o[V];
    unpack16<T>(ld16(x + (row0 + p) * ldx + vc * V), f);
#pragma unroll
    for (int i = 0; i < V; ++i) o[i] = (f[i] - mu[i]) * sc[i] + sh[i];
    if (res) {
      unpack16<T>(ld16(res + (row0 + p) * ldr + vc * V), f);
#pragma unroll
      for (int i = 0; i < V; ++i) o[i] += f[i];
    }
    if (relu) {
#pragma unroll
      for (int i = 0; i < V; ++i) o[i] = fmaxf(o[i], 0.f);
    }
    st16(y + (row0 + p) * ldy + vc * V, pack16<T>(o));
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int tile_pixels(int C) { return GN_TILE_ELEMS / C; }

template <typename T, int NG>
int launch_both(const GroupNormArgs& a, bool stats, hipStream_t s) {
  const int HW = a.H * a.W, PT = tile_pixels(a.C), tiles = spe_gn_tiles(a.H, a.W, a.C);
  const dim3 grid(tiles, a.B);
  if (stats)
    gn_stats_kernel<T, NG><<<grid, GN_THREADS, 0, s>>>((const T*)a.x, a.ldx, a.part, HW, a.C, PT, tiles);
  else
    gn_apply_kernel<T, NG><<<grid, GN_THREADS, 0, s>>>((const T*)a.x, a.ldx, (const T*)a.res, a.ldr, a.gamma, a.beta,
                                                       (T*)a.y, a.ldy, a.part, HW, a.C, PT, tiles, a.relu);
  return (int)hipGetLastError();
}

int launch(const GroupNormArgs& a, int dtype, bool stats, hipStream_t s) {
  if (spe_gn_check(a, dtype)) return -1;
  const int cpg = a.C / GN_GROUPS;
  if (dtype == SPE_DTYPE_BF16)
    return cpg == 2 ? launch_both<bf16, 4>(a, stats, s) : cpg == 4 ? launch_both<bf16, 2>(a, stats, s)
                                                                   : launch_both<bf16, 1>(a, stats, s);
  return cpg == 2 ? launch_both<float, 2>(a, stats, s) : launch_both<float, 1>(a, stats, s);
}

}  // namespace

int spe_gn_tiles(int H, int W, int C) {
  if (H <= 0 || W <= 0 || C <= 0 || C > GN_TILE_ELEMS) return 0;
  const int PT = tile_pixels(C);
  return (int)(((int64_t)H * W + PT - 1) / PT);
}

int64_t spe_gn_scratch_bytes(int B, int H, int W, int C) {
  return (int64_t)B * spe_gn_tiles(H, W, C) * GN_GROUPS * 3 * 4;
}

const char* spe_gn_check(const GroupNormArgs& a, int dtype) {
  if (dtype != SPE_DTYPE_BF16 && dtype != SPE_DTYPE_F32) return "groupnorm: dtype bf16 or fp32";
  if (a.B <= 0 || a.H <= 0 || a.W <= 0 || a.B > 65535 || (int64_t)a.H * a.W > (1 << 30)) return "groupnorm: bad B, H or W";
  if (a.C <= 0 || a.C % GN_GROUPS) return "groupnorm: C must be a multiple of 32";
  const int cpg = a.C / GN_GROUPS;
  if (cpg != 2 && cpg != 4 && cpg != 8 && cpg != 16 && cpg != 32)
    return "groupnorm: C / 32 must be 2, 4, 8, 16 or 32 (C = 64 ... 1024)";
  if (!a.x || !a.y || !a.gamma || !a.beta || !a.part) return "groupnorm: null pointer";
  if (a.ldx < a.C || a.ldx % 8 || a.ldy < a.C || a.ldy % 8) return "groupnorm: ld below C or not a multiple of 8";
  if (a.res && (a.ldr < a.C || a.ldr % 8)) return "groupnorm: residual ld below C or not a multiple of 8";
  if (!aligned16(a.x) || !aligned16(a.y) || !aligned16(a.res) || !aligned16(a.part))
    return "groupnorm: pointers must be 16-byte aligned";
  return nullptr;
}

int spe_launch_gn_stats(const GroupNormArgs& a, int dtype, hipStream_t s) { return launch(a, dtype, true, s); }
int spe_launch_gn_apply(const GroupNormArgs& a, int dtype, hipStream_t s) { return launch(a, dtype, false, s); }
