// What the 2-D and the 3-D discriminator kernels share (csrc/disc_conv3.h, csrc/disc_conv3d.h; csrc/disc.hip, csrc/disc3d.hip): the
// 16x16 pixel tile of one plane ([N][H][W][C] image or [N T][H][W][C] frame) on v_mfma_f32_32x32x2_f32, 256 threads per workgroup.
// The kernels decode blockIdx, pick the prologue vectors and run their loop nest over these parts; every floating-point operation
// is written once, here, in the order the results' bits depend on.
//
//   conv (forward and data gradient): M = the 256 pixels of the tile (wave w owns tile rows 4w .. 4w + 3 = two 32-pixel MFMA row
//     blocks), N = 32 NB output channels, K = taps x Cin in chunks of DISC_KC channels.  The operand is activated while it is staged
//     into LDS (the prologue a = lrelu_0.2(x s[c] + t[c])); positions outside the plane are 0 AFTER the activation.
//   weight gradient: M = 32 input channels, N = 32 output channels, K = the pixels of the tile (wave w owns its 64), one
//     accumulator block per tap; a workgroup walks its work items in order and writes one slab.
//
// LDS (160 KB per CU): the conv holds ONE stage of 18 x 18 x 16 channels (pitch 17: 22 KB) and 9 x 16 x 32 NB weights (18 KB at
// NB = 1, 54 KB at NB = 2 with the row pitch 96 that keeps the two half-waves on disjoint banks): 40 / 76 KB, so two to four
// workgroups share a CU and one's staging overlaps another's MFMAs -- the second stage is another resident workgroup.
// The weight gradient holds 18 x 18 x 32 channels (pitch 33: 42 KB) and the 256 x 32 tile of dy (32 KB): 74 KB, two per CU.
// Operands whose channel count is a multiple of 32 are staged with 16-byte loads, a thread's loads issued before the first is
// used (disc_stage_halo_vec); the 1..8-channel ends of the nets take the scalar path (disc_stage_halo).  Same bits either way.
// The stride-2 stem of the 3-D net stages (15 S + 3)^2 positions at pitch 9 instead (disc_conv3d.h): <S, HS, AP> below.
#pragma once
#include "oniris.h"
#include "common.h"

#define DISC_TILE 16
#define DISC_HALO 18
#define DISC_KC 16
#define DISC_APITCH 17
#define DISC_WKC 32
#define DISC_WPITCH 33
#define DISC_SLOPE 0.2f
#define DISC_RED_PIX 1024                                         // pixels per workgroup of the norm-backward reduce

__device__ __forceinline__ float disc_act(float x, float s, float t) {
  const float z = __builtin_fmaf(x, s, t);
  return z > 0.f ? z : z * DISC_SLOPE;
}

// dz = da lrelu'(z s + t)
__device__ __forceinline__ float disc_dz(float z, float s, float t, float g) {
  return __builtin_fmaf(z, s, t) > 0.f ? g : g * DISC_SLOPE;
}

// The 18 x 18 halo of tile (y0, x0) of plane n, channels c0 .. c0 + kc - 1, into hl[pixel * PITCH + c]; channels >= Cin and
// positions outside the plane are 0.
template <int PITCH>
__device__ __forceinline__ void disc_stage_halo(float* hl, const float* __restrict__ x, const float* __restrict__ pro_s,
                                                const float* __restrict__ pro_t, int n, int y0, int x0, int H, int W, int Cin, int c0,
                                                int kc) {
  const int total = DISC_HALO * DISC_HALO * kc;
  for (int idx = threadIdx.x; idx < total; idx += 256) {
    const int c = idx % kc, pix = idx / kc;
    const int y = y0 - 1 + pix / DISC_HALO, xx = x0 - 1 + pix % DISC_HALO;
    float v = 0.f;
    if (y >= 0 && y < H && xx >= 0 && xx < W && c0 + c < Cin) {
      v = x[(((size_t)n * H + y) * W + xx) * Cin + c0 + c];
      if (pro_s) v = disc_act(v, pro_s[c0 + c], pro_t[c0 + c]);
    }
    hl[pix * PITCH + c] = v;
  }
}

// The same for a full chunk of KC channels of a tensor whose channel count is a multiple of 32: 16-byte loads, all of a thread's
// loads issued before the first is used.  Bit for bit what disc_stage_halo stores.
template <int PITCH, int KC>
__device__ __forceinline__ void disc_stage_halo_vec(float* hl, const float* __restrict__ x, const float* __restrict__ pro_s,
                                                    const float* __restrict__ pro_t, int n, int y0, int x0, int H, int W, int Cin,
                                                    int c0) {
  constexpr int Q = KC / 4, TOTAL = DISC_HALO * DISC_HALO * Q, IT = (TOTAL + 255) / 256;
  f32x4 v[IT];
  bool in[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int idx = threadIdx.x + it * 256;
    const int q = idx % Q, pix = idx / Q;
    const int y = y0 - 1 + pix / DISC_HALO, xx = x0 - 1 + pix % DISC_HALO;
    in[it] = idx < TOTAL && y >= 0 && y < H && xx >= 0 && xx < W;
    v[it] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (in[it]) v[it] = *reinterpret_cast<const f32x4*>(x + (((size_t)n * H + y) * W + xx) * Cin + c0 + 4 * q);
  }
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int idx = threadIdx.x + it * 256;
    if (idx >= TOTAL) break;
    const int q = idx % Q, pix = idx / Q;
    float* o = hl + pix * PITCH + 4 * q;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float a = v[it][e];
      if (pro_s && in[it]) a = disc_act(a, pro_s[c0 + 4 * q + e], pro_t[c0 + 4 * q + e]);
      o[e] = a;
    }
  }
}

template <int N>
__device__ __forceinline__ void disc_zero(f32x16 (&acc)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
}

// ---- conv

template <int NB>
__device__ __forceinline__ void disc_zero(f32x16 (&acc)[2][NB]) {
  disc_zero(acc[0]);
  disc_zero(acc[1]);
}

// Taps tap0 .. tap0 + ntaps - 1 of w[tap][CinP][CoutP], channels c0 .. c0 + kc - 1, output channels n0 .. n0 + 32 NB - 1, into
// wl[tap - tap0][16][WP].
template <int NB>
__device__ __forceinline__ void disc_stage_weights(float* wl, const float* w, int tap0, int ntaps, int CinP, int CoutP, int c0, int kc,
                                                   int n0) {
  constexpr int WN = 32 * NB, WP = (NB & 1) ? WN : WN + 32;
#pragma unroll 4
  for (int idx = threadIdx.x; idx < ntaps * kc * (WN / 4); idx += 256) {
    const int jq = idx % (WN / 4), c = (idx / (WN / 4)) % kc, tp = idx / ((WN / 4) * kc);
    *reinterpret_cast<f32x4*>(wl + (tp * DISC_KC + c) * WP + 4 * jq) =
        *reinterpret_cast<const f32x4*>(w + ((size_t)(tap0 + tp) * CinP + c0 + c) * CoutP + n0 + 4 * jq);
  }
}

// Epilogue of tile (y0, x0) of output plane `plane` ([.][Ho][Wo][Cout]), output channels n0 .. n0 + 32 NB - 1: + bias,
// (v + res) * scale, masked store; with `part`, the workgroup's statistics of what it stored.  lds: the workgroup's LDS, free.
template <int NB>
__device__ __forceinline__ void disc_epilogue(f32x16 (&acc)[2][NB], float* lds, int plane, int Ho, int Wo, int y0, int x0, int n0,
                                              int Cout, const float* bias, const float* res, float res_scale, float* out, float* part) {
  constexpr int WN = 32 * NB;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, kh = lane >> 5;
  // acc keeps the stored values for the statistics
  float lsum[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int co = n0 + nb * 32 + j;
    const float bv = (bias && co < Cout) ? bias[co] : 0.f;
    lsum[nb] = 0.f;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = mfma_row(r, lane);
        const int y = y0 + 4 * wave + 2 * mb + (i >> 4), xx = x0 + (i & 15);
        const bool ok = y < Ho && xx < Wo && co < Cout;
        float v = acc[mb][nb][r] + bv;
        if (ok) {
          const size_t o = (((size_t)plane * Ho + y) * Wo + xx) * Cout + co;
          if (res) v = (v + res[o]) * res_scale;
          out[o] = v;
          lsum[nb] += v;
        }
        acc[mb][nb][r] = v;
      }
  }
  if (!part) return;

  // per-workgroup (count, centre, S2, S1) of the stored values: centre = the tile's own mean rounded to fp32, S2 / S1 = the sums of
  // (v - centre)^2 and of v - centre (each difference is exact or nearly so).  The tile's mean is centre + S1 / count: the fp32
  // rounding of a mean far from 0 would otherwise enter the between-tile term of Chan's formula.
  float* red = lds;                                              // [2][8][WN]
  float* mean_l = lds + 16 * WN;                                 // [WN]
  const float cnt = (float)(min(DISC_TILE, Ho - y0) * min(DISC_TILE, Wo - x0));
  __syncthreads();
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) red[(2 * wave + kh) * WN + nb * 32 + j] = lsum[nb];
  __syncthreads();
  if (threadIdx.x < WN) {
    float s = 0.f;
    for (int q = 0; q < 8; ++q) s += red[q * WN + threadIdx.x];
    mean_l[threadIdx.x] = s / cnt;
  }
  __syncthreads();
  float lq1[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int co = n0 + nb * 32 + j;
    const float m = mean_l[nb * 32 + j];
    float q1 = 0.f, q2 = 0.f;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = mfma_row(r, lane);
        const int y = y0 + 4 * wave + 2 * mb + (i >> 4), xx = x0 + (i & 15);
        if (y < Ho && xx < Wo && co < Cout) {
          const float d = acc[mb][nb][r] - m;
          q1 += d;
          q2 = __builtin_fmaf(d, d, q2);
        }
      }
    lsum[nb] = q2;
    lq1[nb] = q1;
  }
  __syncthreads();
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    red[(2 * wave + kh) * WN + nb * 32 + j] = lsum[nb];
    red[(8 + 2 * wave + kh) * WN + nb * 32 + j] = lq1[nb];
  }
  __syncthreads();
  if (threadIdx.x < WN && n0 + threadIdx.x < Cout) {
    float s2 = 0.f, s1 = 0.f;
    for (int q = 0; q < 8; ++q) {
      s2 += red[q * WN + threadIdx.x];
      s1 += red[(8 + q) * WN + threadIdx.x];
    }
    float* o = part + (size_t)blockIdx.x * 4 * Cout + n0 + threadIdx.x;
    o[0] = cnt;
    o[Cout] = mean_l[threadIdx.x];
    o[2 * Cout] = s2;
    o[3 * Cout] = s1;
  }
}

// ---- weight gradient

// Tile (y0, x0) of plane `plane` of dy ([.][Ho][Wo][Cout]), channels co0 .. co0 + 31, into dyl[256][32]; 0 outside.
__device__ __forceinline__ void disc_stage_dy(float* dyl, const float* dy, int plane, int y0, int x0, int Ho, int Wo,
                                              int Cout, int co0) {
  if (Cout % 32 == 0) {
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int idx = threadIdx.x + it * 256, c4 = idx & 7, pix = idx >> 3;
      const int y = y0 + (pix >> 4), xx = x0 + (pix & 15);
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (y < Ho && xx < Wo) v = *reinterpret_cast<const f32x4*>(dy + (((size_t)plane * Ho + y) * Wo + xx) * Cout + co0 + 4 * c4);
      *reinterpret_cast<f32x4*>(dyl + 4 * idx) = v;
    }
  } else {
    for (int idx = threadIdx.x; idx < 256 * 32; idx += 256) {
      const int co = idx & 31, pix = idx >> 5;
      const int y = y0 + (pix >> 4), xx = x0 + (pix & 15);
      float v = 0.f;
      if (y < Ho && xx < Wo && co0 + co < Cout) v = dy[(((size_t)plane * Ho + y) * Wo + xx) * Cout + co0 + co];
      dyl[idx] = v;
    }
  }
}

// One staged tile: TAPS = 9, or 1 = the centre tap (1, 1); hl[HS * HS][AP] as in disc_mfma_taps, its channels >= kc read as 0.
template <int TAPS, int S, int HS, int AP>
__device__ __forceinline__ void disc_wgrad_mfma(f32x16 (&acc)[TAPS], const float* hl, const float* dyl, int kc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, kh = lane >> 5;
  for (int s = 0; s < 32; ++s) {
    const int pi = 2 * s + kh, prow = 4 * wave + (pi >> 4), pcol = pi & 15;
    const float b = dyl[(prow * 16 + pcol) * 32 + j];
#pragma unroll
    for (int tp = 0; tp < TAPS; ++tp) {
      const int ky = TAPS == 9 ? tp / 3 : 1, kx = TAPS == 9 ? tp % 3 : 1;
      const float a = j < kc ? hl[((prow * S + ky) * HS + pcol * S + kx) * AP + j] : 0.f;
      acc[tp] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[tp], 0, 0, 0);
    }
  }
}

// The bias gradient's share of one staged tile: thread (q, co) adds the 32 pixels q 32 .. q 32 + 31 of channel co.
__device__ __forceinline__ void disc_bias_rows(float& bsum, const float* dyl) {
  const int co = threadIdx.x & 31, q = threadIdx.x >> 5;
  for (int k = 0; k < 32; ++k) bsum += dyl[(q * 32 + k) * 32 + co];
}

// The four waves' accumulators summed through hl, wave 0 first, into taps tap0 .. tap0 + TAPS - 1 of slab[taps_total][Cin][Cout];
// the workgroup that owns the bias adds its row sums through dyl and writes them behind the weights, at row bias_off / Cout of a
// bias that has several (the wide VAE's [gl][C] and [sub][C]).
template <int TAPS>
__device__ __forceinline__ void disc_wgrad_store(const f32x16 (&acc)[TAPS], float bsum, float* hl, float* dyl, float* slab,
                                                 int tap0, int taps_total, bool bias_wg, int Cin, int Cout, int ci0, int co0,
                                                 size_t bias_off = 0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31;
  __syncthreads();
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int idx = tp * 1024 + mfma_row(r, lane) * 32 + j;
          hl[idx] = w == 0 ? acc[tp][r] : hl[idx] + acc[tp][r];
        }
    }
    __syncthreads();
  }
  for (int idx = threadIdx.x; idx < TAPS * 1024; idx += 256) {
    const int co = idx & 31, ci = (idx >> 5) & 31, tp = idx >> 10;
    if (ci0 + ci < Cin && co0 + co < Cout) slab[((size_t)(tap0 + tp) * Cin + ci0 + ci) * Cout + co0 + co] = hl[idx];
  }
  if (bias_wg) {
    dyl[threadIdx.x] = bsum;                                     // [q][co]
    __syncthreads();
    if (threadIdx.x < 32 && co0 + threadIdx.x < Cout) {
      float s = 0.f;
      for (int q = 0; q < 8; ++q) s += dyl[q * 32 + threadIdx.x];
      slab[(size_t)taps_total * Cin * Cout + bias_off + co0 + threadIdx.x] = s;
    }
  }
}

// ---- statistics: Chan's combination of (count, mean, M2) in double (the partials are fp32; a handful of values per channel)
__device__ __forceinline__ void disc_chan(double& n, double& m, double& q, double nb, double mb, double qb) {
  if (nb == 0.0) return;
  if (n == 0.0) { n = nb; m = mb; q = qb; return; }
  const double tot = n + nb, d = mb - m;
  m = m + d * (nb / tot);
  q = q + qb + d * d * (n * (nb / tot));
  n = tot;
}

// Norm + LeakyReLU backward, the reduce: per workgroup (DISC_RED_PIX positions of sample blockIdx.z, 32 channels) the sums of dz
// and dz xhat into part[sample][workgroup][2][C].  stats = [mean | var | s | t | rstd][N][C]; BatchNorm is N = 1, gridDim.z = 1.
// (A template so that both translation units may hold it.)
template <int PIX>
__global__ __launch_bounds__(256) void disc3d_gn_bwd_reduce_kernel(const float* __restrict__ da, const float* __restrict__ z,
                                                                   const float* __restrict__ stats, float* __restrict__ part, int N,
                                                                   long long npix, int C) {
  __shared__ float r1[256], r2[256];
  const int cl = threadIdx.x & 31, q = threadIdx.x >> 5, c = blockIdx.y * 32 + cl, smp = blockIdx.z;
  const bool live = c < C;
  float s1 = 0.f, s2 = 0.f;
  if (live) {
    const size_t NC = (size_t)N * C, o = (size_t)smp * C + c;
    const float mean = stats[o], s = stats[2 * NC + o], t = stats[3 * NC + o], rstd = stats[4 * NC + o];
    const long long p0 = (long long)blockIdx.x * PIX + q * (PIX / 8);
    const float* zb = z + (size_t)smp * npix * C;
    const float* db = da + (size_t)smp * npix * C;
    for (int k = 0; k < PIX / 8; ++k) {
      const long long pix = p0 + k;
      if (pix >= npix) break;
      const float zv = zb[pix * C + c];
      const float dz = disc_dz(zv, s, t, db[pix * C + c]);
      s1 += dz;
      s2 = __builtin_fmaf(dz, (zv - mean) * rstd, s2);
    }
  }
  r1[threadIdx.x] = s1; r2[threadIdx.x] = s2;
  __syncthreads();
  if (threadIdx.x < 32 && live) {
    float a = 0.f, b = 0.f;
    for (int k = 0; k < 8; ++k) { a += r1[k * 32 + cl]; b += r2[k * 32 + cl]; }
    float* o = part + ((size_t)smp * gridDim.x + blockIdx.x) * 2 * C;
    o[c] = a;
    o[C + c] = b;
  }
}

// ---- host side

template <typename K>
static int disc_raise_lds(K kern, size_t bytes, const char* what) {
  if (bytes <= 64 * 1024) return ONIRIS_OK;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) {
    oniris_set_error("%s: raising the LDS limit failed: %s", what, hipGetErrorString(e));
    return ONIRIS_ELAUNCH;
  }
  return ONIRIS_OK;
}

static inline bool disc_c_ok(int c) { return (c >= 1 && c <= 8) || (c > 0 && c % 32 == 0); }    // a channel count the kernels take
static inline int disc_out(int n, int stride) { return (n - 1) / stride + 1; }                  // extent after kernel 3, padding 1

static inline int disc3d_gn_bwd_reduce_launch(const char* what, const float* da, const float* z, const float* stats, float* part,
                                              int N, long long npix, int C, hipStream_t stream) {
  const long long P = (npix + DISC_RED_PIX - 1) / DISC_RED_PIX;
  ONIRIS_CHECK_ARG(P <= 0x7fffffffLL, "%s: %lld positions", what, npix);
  ONIRIS_KLAUNCH(disc3d_gn_bwd_reduce_kernel<DISC_RED_PIX>, dim3((unsigned)P, cdiv(C, 32), N), dim3(256), 0, stream, da, z, stats, part, N,
                 npix, C);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}
