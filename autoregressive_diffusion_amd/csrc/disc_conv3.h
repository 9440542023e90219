// The discriminator's fp32 implicit-GEMM convolutions on v_mfma_f32_32x32x2_f32 (reference: edm2/vae/discriminator.py, the
// nn.Conv2d of DiscriminatorBlock2D / Discriminator2D).  Channels-last fp32 [N][H][W][C]; one workgroup of 256 threads per
// 16x16 pixel tile.
//
//   disc_conv_kernel<NB>   forward and data gradient, 3x3 (zero padding 1) or 1x1: M = the 256 pixels of the tile (wave w owns
//                          tile rows 4w .. 4w + 3 = two 32-pixel MFMA row blocks), N = 32 NB output channels, K = taps x Cin in
//                          chunks of DISC_KC channels.  The operand is activated while it is staged into LDS (the prologue
//                          a = lrelu_0.2(x s[c] + t[c])); positions outside the image are 0 AFTER the activation.
//   disc_wgrad_kernel<T>   weight and bias gradient: M = 32 input channels, N = 32 output channels, K = the pixels of the tile
//                          (wave w owns its 64), one accumulator block per tap; workgroup s walks the work items (image, tile)
//                          s, s + nslab, ... in that order and writes slab s.
//
// LDS (160 KB per CU): the forward holds ONE stage of 18 x 18 x 16 channels (pitch 17: 22 KB) and 9 x 16 x 32 NB weights (18 KB at
// NB = 1, 54 KB at NB = 2 with the row pitch 96 that keeps the two half-waves on disjoint banks): 40 / 76 KB, so two to four
// workgroups share a CU and one's staging overlaps another's MFMAs -- the second stage is another resident workgroup.
// The weight gradient holds 18 x 18 x 32 channels (pitch 33: 42 KB) and the 256 x 32 tile of dy (32 KB): 74 KB, two per CU.
// Operands whose channel count is a multiple of 32 are staged with 16-byte loads, a thread's loads issued before the first is
// used (disc_stage_halo_vec); the 1..8-channel ends of the net take the scalar path (disc_stage_halo).  Same bits either way.
#pragma once
#include "common.h"

#define DISC_TILE 16
#define DISC_HALO 18
#define DISC_KC 16
#define DISC_APITCH 17
#define DISC_WKC 32
#define DISC_WPITCH 33
#define DISC_SLOPE 0.2f

__device__ __forceinline__ float disc_act(float x, float s, float t) {
  const float z = __builtin_fmaf(x, s, t);
  return z > 0.f ? z : z * DISC_SLOPE;
}

// The 18 x 18 halo of tile (y0, x0) of image n, channels c0 .. c0 + kc - 1, into hl[pixel * PITCH + c]; channels >= Cin and
// positions outside the image are 0.
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

struct DiscConvParams {
  const float* x; const float* w; const float* bias; const float* pro_s; const float* pro_t; const float* res;
  float* out; float* part;
  int N, H, W, Cin, CinP, Cout, CoutP, taps, tiles_x, tiles_y;
  float res_scale;
};

template <int NB>
__global__ __launch_bounds__(256) void disc_conv_kernel(DiscConvParams p) {
  constexpr int WN = 32 * NB, WP = (NB & 1) ? WN : WN + 32;
  extern __shared__ __attribute__((aligned(16))) float disc_lds[];
  float* hl = disc_lds;                                          // [324][17]
  float* wl = disc_lds + DISC_HALO * DISC_HALO * DISC_APITCH;    // [taps][16][WP]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, kh = lane >> 5;
  const int tile = blockIdx.x % (p.tiles_x * p.tiles_y), n = blockIdx.x / (p.tiles_x * p.tiles_y);
  const int y0 = (tile / p.tiles_x) * DISC_TILE, x0 = (tile % p.tiles_x) * DISC_TILE;
  const int n0 = blockIdx.y * WN;
  const int prow = 4 * wave + (j >> 4), pcol = j & 15;           // the lane's A pixel in row block 0; row block 1: prow + 2

  f32x16 acc[2][NB];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;

  for (int c0 = 0; c0 < p.CinP; c0 += DISC_KC) {
    const int kc = min(DISC_KC, p.CinP - c0);
    __syncthreads();
    if (p.Cin % 32 == 0) disc_stage_halo_vec<DISC_APITCH, DISC_KC>(hl, p.x, p.pro_s, p.pro_t, n, y0, x0, p.H, p.W, p.Cin, c0);
    else disc_stage_halo<DISC_APITCH>(hl, p.x, p.pro_s, p.pro_t, n, y0, x0, p.H, p.W, p.Cin, c0, kc);
#pragma unroll 4
    for (int idx = threadIdx.x; idx < p.taps * kc * (WN / 4); idx += 256) {
      const int jq = idx % (WN / 4), c = (idx / (WN / 4)) % kc, tp = idx / ((WN / 4) * kc);
      *reinterpret_cast<f32x4*>(wl + (tp * DISC_KC + c) * WP + 4 * jq) =
          *reinterpret_cast<const f32x4*>(p.w + ((size_t)tp * p.CinP + c0 + c) * p.CoutP + n0 + 4 * jq);
    }
    __syncthreads();
    for (int tp = 0; tp < p.taps; ++tp) {
      const int ky = p.taps == 9 ? tp / 3 : 1, kx = p.taps == 9 ? tp % 3 : 1;
      const float* a0p = hl + ((prow + ky) * DISC_HALO + pcol + kx) * DISC_APITCH + kh;
      const float* a1p = a0p + 2 * DISC_HALO * DISC_APITCH;
      const float* bp = wl + (tp * DISC_KC + kh) * WP + j;
      for (int kk = 0; kk < kc; kk += 2) {
        const float a0 = a0p[kk], a1 = a1p[kk];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          const float b = bp[kk * WP + nb * 32];
          acc[0][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0][nb], 0, 0, 0);
          acc[1][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1][nb], 0, 0, 0);
        }
      }
    }
  }

  // epilogue: + bias, (v + res) * scale, masked store; acc keeps the stored values for the statistics
  float lsum[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int co = n0 + nb * 32 + j;
    const float bv = (p.bias && co < p.Cout) ? p.bias[co] : 0.f;
    lsum[nb] = 0.f;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = mfma_row(r, lane);
        const int y = y0 + 4 * wave + 2 * mb + (i >> 4), xx = x0 + (i & 15);
        const bool ok = y < p.H && xx < p.W && co < p.Cout;
        float v = acc[mb][nb][r] + bv;
        if (ok) {
          const size_t o = (((size_t)n * p.H + y) * p.W + xx) * p.Cout + co;
          if (p.res) v = (v + p.res[o]) * p.res_scale;
          p.out[o] = v;
          lsum[nb] += v;
        }
        acc[mb][nb][r] = v;
      }
  }
  if (!p.part) return;

  // per-workgroup (count, centre, S2, S1) of the stored values: centre = the tile's own mean rounded to fp32, S2 / S1 = the sums of
  // (v - centre)^2 and of v - centre (each difference is exact or nearly so).  The tile's mean is centre + S1 / count: the fp32
  // rounding of a mean far from 0 would otherwise enter the between-tile term of Chan's formula.
  float* red = disc_lds;                                         // [2][8][WN]
  float* mean_l = disc_lds + 16 * WN;                            // [WN]
  const float cnt = (float)(min(DISC_TILE, p.H - y0) * min(DISC_TILE, p.W - x0));
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
        if (y < p.H && xx < p.W && co < p.Cout) {
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
  if (threadIdx.x < WN && n0 + threadIdx.x < p.Cout) {
    float s2 = 0.f, s1 = 0.f;
    for (int q = 0; q < 8; ++q) {
      s2 += red[q * WN + threadIdx.x];
      s1 += red[(8 + q) * WN + threadIdx.x];
    }
    float* o = p.part + (size_t)blockIdx.x * 4 * p.Cout + n0 + threadIdx.x;
    o[0] = cnt;
    o[p.Cout] = mean_l[threadIdx.x];
    o[2 * p.Cout] = s2;
    o[3 * p.Cout] = s1;
  }
}

struct DiscWgradParams {
  const float* x; const float* pro_s; const float* pro_t; const float* dy;
  float* slab;
  int N, H, W, Cin, CinP, Cout, tiles_x, tiles_y, nitems, nslab;
  long long slab_size;
};

template <int TAPS>
__global__ __launch_bounds__(256) void disc_wgrad_kernel(DiscWgradParams p) {
  extern __shared__ __attribute__((aligned(16))) float disc_lds[];
  float* hl = disc_lds;                                                  // [324][33]; afterwards the cross-wave sum [TAPS][32][32]
  float* dyl = disc_lds + DISC_HALO * DISC_HALO * DISC_WPITCH;           // [256][32]; afterwards the bias sums [8][32]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, kh = lane >> 5;
  const int ci0 = blockIdx.y * DISC_WKC, co0 = blockIdx.z * 32;
  const int kc = min(DISC_WKC, p.CinP - ci0);
  const int tiles = p.tiles_x * p.tiles_y;

  f32x16 acc[TAPS];
#pragma unroll
  for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[tp][r] = 0.f;
  float bsum = 0.f;

  for (int item = blockIdx.x; item < p.nitems; item += p.nslab) {
    const int n = item / tiles, tile = item % tiles;
    const int y0 = (tile / p.tiles_x) * DISC_TILE, x0 = (tile % p.tiles_x) * DISC_TILE;
    __syncthreads();
    if (p.Cin % 32 == 0) disc_stage_halo_vec<DISC_WPITCH, DISC_WKC>(hl, p.x, p.pro_s, p.pro_t, n, y0, x0, p.H, p.W, p.Cin, ci0);
    else disc_stage_halo<DISC_WPITCH>(hl, p.x, p.pro_s, p.pro_t, n, y0, x0, p.H, p.W, p.Cin, ci0, kc);
    if (p.Cout % 32 == 0) {
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int idx = threadIdx.x + it * 256, c4 = idx & 7, pix = idx >> 3;
        const int y = y0 + (pix >> 4), xx = x0 + (pix & 15);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (y < p.H && xx < p.W) v = *reinterpret_cast<const f32x4*>(p.dy + (((size_t)n * p.H + y) * p.W + xx) * p.Cout + co0 + 4 * c4);
        *reinterpret_cast<f32x4*>(dyl + 4 * idx) = v;
      }
    } else {
      for (int idx = threadIdx.x; idx < 256 * 32; idx += 256) {
        const int co = idx & 31, pix = idx >> 5;
        const int y = y0 + (pix >> 4), xx = x0 + (pix & 15);
        float v = 0.f;
        if (y < p.H && xx < p.W && co0 + co < p.Cout) v = p.dy[(((size_t)n * p.H + y) * p.W + xx) * p.Cout + co0 + co];
        dyl[idx] = v;
      }
    }
    __syncthreads();
    for (int s = 0; s < 32; ++s) {
      const int pi = 2 * s + kh, prow = 4 * wave + (pi >> 4), pcol = pi & 15;
      const float b = dyl[(prow * 16 + pcol) * 32 + j];
#pragma unroll
      for (int tp = 0; tp < TAPS; ++tp) {
        const int ky = TAPS == 9 ? tp / 3 : 1, kx = TAPS == 9 ? tp % 3 : 1;
        const float a = j < kc ? hl[((prow + ky) * DISC_HALO + pcol + kx) * DISC_WPITCH + j] : 0.f;
        acc[tp] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[tp], 0, 0, 0);
      }
    }
    if (blockIdx.y == 0) {
      const int co = threadIdx.x & 31, q = threadIdx.x >> 5;
      for (int k = 0; k < 32; ++k) bsum += dyl[(q * 32 + k) * 32 + co];
    }
  }

  // the four waves' accumulators, wave 0 first
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
  float* slab = p.slab + (size_t)blockIdx.x * p.slab_size;
  for (int idx = threadIdx.x; idx < TAPS * 1024; idx += 256) {
    const int co = idx & 31, ci = (idx >> 5) & 31, tp = idx >> 10;
    if (ci0 + ci < p.Cin && co0 + co < p.Cout) slab[((size_t)tp * p.Cin + ci0 + ci) * p.Cout + co0 + co] = hl[idx];
  }
  if (blockIdx.y == 0) {
    dyl[threadIdx.x] = bsum;                                             // [q][co]
    __syncthreads();
    if (threadIdx.x < 32 && co0 + threadIdx.x < p.Cout) {
      float s = 0.f;
      for (int q = 0; q < 8; ++q) s += dyl[q * 32 + threadIdx.x];
      slab[(size_t)TAPS * p.Cin * p.Cout + co0 + threadIdx.x] = s;
    }
  }
}
