// The 3-D discriminator's fp32 implicit-GEMM convolutions on v_mfma_f32_32x32x2_f32 (reference: edm2/vae/discriminator.py, the
// nn.Conv3d of DiscriminatorBlock3D / Discriminator3D).  Channels-last fp32 [N][T][H][W][C]; a 27-tap conv is the sum over kt of
// three 9-tap convs of the planes t S + kt - 1, so the 16x16 tile, the halo stage and the inner loop of csrc/disc_conv3.h carry over
// with one more loop level; planes outside 0 .. T - 1 are skipped.  One workgroup of 256 threads per 16x16 tile of one output
// plane of one sample: a tile never spans two samples, and the prologue vectors are per (sample, channel).
//
//   disc3d_conv_kernel<NB, S>   S = 1: forward and data gradient of the 27-tap convs, zero padding 1, operand staged by
//                               disc_stage_halo(_vec) -- LDS as the 2-D kernel's.  S = 2: the stem conv_in, stride 2 in T, H and W,
//                               1..8 input channels padded to 8: the stage is the 33 x 33 input positions a tile of outputs reads
//                               (pitch 9: 38 KB), output position (y, x) tap (ky, kx) reads stage position (2 y + ky, 2 x + kx).
//   disc3d_wgrad_kernel<S>      weight and bias gradient: blockIdx.y carries kt and the 32-channel block of Cin, so a workgroup
//                               holds the 9 accumulator blocks of one kt and pairs plane t S + kt - 1 of the operand with plane t of
//                               dy; workgroup s walks the work items (sample, plane, tile) s, s + nslab, ... and writes slab s.
#pragma once
#include "common.h"
#include "disc_conv3.h"

// The (15 S + 3)^2 input positions of the output tile (y0, x0) of plane `plane` (= n T + t), channels 0 .. kc - 1, no prologue.
template <int S, int PITCH>
__device__ __forceinline__ void disc3d_stage_halo_strided(float* hl, const float* __restrict__ x, long long plane, int y0, int x0,
                                                          int H, int W, int Cin, int kc) {
  constexpr int HS = 15 * S + 3;
  const int total = HS * HS * kc;
  for (int idx = threadIdx.x; idx < total; idx += 256) {
    const int c = idx % kc, pix = idx / kc;
    const int y = y0 * S - 1 + pix / HS, xx = x0 * S - 1 + pix % HS;
    float v = 0.f;
    if (y >= 0 && y < H && xx >= 0 && xx < W && c < Cin) v = x[(((size_t)plane * H + y) * W + xx) * Cin + c];
    hl[pix * PITCH + c] = v;
  }
}

struct Disc3dConvParams {
  const float* x; const float* w; const float* bias; const float* pro_s; const float* pro_t; const float* res;
  float* out; float* part;
  int N, T, H, W, To, Ho, Wo, Cin, CinP, Cout, CoutP, tiles_x, tiles_y;
  float res_scale;
};

template <int NB, int S>
__global__ __launch_bounds__(256) void disc3d_conv_kernel(Disc3dConvParams p) {
  constexpr int WN = 32 * NB, WP = (NB & 1) ? WN : WN + 32;
  constexpr int HS = 15 * S + 3, AP = S == 1 ? DISC_APITCH : 9;
  extern __shared__ __attribute__((aligned(16))) float disc_lds[];
  float* hl = disc_lds;                                          // [HS * HS][AP]
  float* wl = disc_lds + HS * HS * AP;                           // [9][16][WP]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, kh = lane >> 5;
  const int tiles = p.tiles_x * p.tiles_y;
  const int tile = blockIdx.x % tiles, plane_o = blockIdx.x / tiles;             // plane_o = n To + to
  const int n = plane_o / p.To, to = plane_o % p.To;
  const int y0 = (tile / p.tiles_x) * DISC_TILE, x0 = (tile % p.tiles_x) * DISC_TILE;
  const int n0 = blockIdx.y * WN;
  const int prow = 4 * wave + (j >> 4), pcol = j & 15;
  const float* ps = p.pro_s ? p.pro_s + (size_t)n * p.Cin : nullptr;
  const float* pt = p.pro_t ? p.pro_t + (size_t)n * p.Cin : nullptr;

  f32x16 acc[2][NB];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;

  for (int kt = 0; kt < 3; ++kt) {
    const int tin = to * S + kt - 1;
    if (tin < 0 || tin >= p.T) continue;                         // a plane of zero padding
    const int plane = n * p.T + tin;
    for (int c0 = 0; c0 < p.CinP; c0 += DISC_KC) {
      const int kc = min(DISC_KC, p.CinP - c0);
      __syncthreads();
      if (S == 1) {
        if (p.Cin % 32 == 0) disc_stage_halo_vec<DISC_APITCH, DISC_KC>(hl, p.x, ps, pt, plane, y0, x0, p.H, p.W, p.Cin, c0);
        else disc_stage_halo<DISC_APITCH>(hl, p.x, ps, pt, plane, y0, x0, p.H, p.W, p.Cin, c0, kc);
      } else {
        disc3d_stage_halo_strided<S, AP>(hl, p.x, plane, y0, x0, p.H, p.W, p.Cin, kc);
      }
#pragma unroll 4
      for (int idx = threadIdx.x; idx < 9 * kc * (WN / 4); idx += 256) {
        const int jq = idx % (WN / 4), c = (idx / (WN / 4)) % kc, tp = idx / ((WN / 4) * kc);
        *reinterpret_cast<f32x4*>(wl + (tp * DISC_KC + c) * WP + 4 * jq) =
            *reinterpret_cast<const f32x4*>(p.w + ((size_t)(kt * 9 + tp) * p.CinP + c0 + c) * p.CoutP + n0 + 4 * jq);
      }
      __syncthreads();
      for (int tp = 0; tp < 9; ++tp) {
        const int ky = tp / 3, kx = tp % 3;
        const float* a0p = hl + ((prow * S + ky) * HS + pcol * S + kx) * AP + kh;
        const float* a1p = a0p + 2 * S * HS * AP;
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
        const bool ok = y < p.Ho && xx < p.Wo && co < p.Cout;
        float v = acc[mb][nb][r] + bv;
        if (ok) {
          const size_t o = (((size_t)plane_o * p.Ho + y) * p.Wo + xx) * p.Cout + co;
          if (p.res) v = (v + p.res[o]) * p.res_scale;
          p.out[o] = v;
          lsum[nb] += v;
        }
        acc[mb][nb][r] = v;
      }
  }
  if (!p.part) return;

  // per-workgroup (count, centre, S2, S1) of the stored values, exactly as disc_conv_kernel emits them
  float* red = disc_lds;                                         // [2][8][WN]
  float* mean_l = disc_lds + 16 * WN;                            // [WN]
  const float cnt = (float)(min(DISC_TILE, p.Ho - y0) * min(DISC_TILE, p.Wo - x0));
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
        if (y < p.Ho && xx < p.Wo && co < p.Cout) {
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

struct Disc3dWgradParams {
  const float* x; const float* pro_s; const float* pro_t; const float* dy;
  float* slab;
  int N, T, H, W, To, Ho, Wo, Cin, CinP, Cout, tiles_x, tiles_y, nitems, nslab, ncib;
  long long slab_size;
};

template <int S>
__global__ __launch_bounds__(256) void disc3d_wgrad_kernel(Disc3dWgradParams p) {
  constexpr int HS = 15 * S + 3, AP = S == 1 ? DISC_WPITCH : 9;
  extern __shared__ __attribute__((aligned(16))) float disc_lds[];
  float* hl = disc_lds;                                          // [HS * HS][AP]; afterwards the cross-wave sum [9][32][32]
  float* dyl = disc_lds + HS * HS * AP;                          // [256][32]; afterwards the bias sums [8][32]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, kh = lane >> 5;
  const int kt = blockIdx.y / p.ncib, ci0 = (blockIdx.y % p.ncib) * DISC_WKC, co0 = blockIdx.z * 32;
  const int kc = min(DISC_WKC, p.CinP - ci0);
  const int tiles = p.tiles_x * p.tiles_y;
  const bool bias_wg = blockIdx.y == p.ncib;                     // kt = 1, the first channel block: its plane always exists

  f32x16 acc[9];
#pragma unroll
  for (int tp = 0; tp < 9; ++tp)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[tp][r] = 0.f;
  float bsum = 0.f;

  for (int item = blockIdx.x; item < p.nitems; item += p.nslab) {
    const int plane_o = item / tiles, tile = item % tiles;
    const int n = plane_o / p.To, to = plane_o % p.To;
    const int tin = to * S + kt - 1;
    if (tin < 0 || tin >= p.T) continue;                         // the same for every thread of the workgroup
    const int plane = n * p.T + tin;
    const int y0 = (tile / p.tiles_x) * DISC_TILE, x0 = (tile % p.tiles_x) * DISC_TILE;
    __syncthreads();
    if (S == 1) {
      const float* ps = p.pro_s ? p.pro_s + (size_t)n * p.Cin : nullptr;
      const float* pt = p.pro_t ? p.pro_t + (size_t)n * p.Cin : nullptr;
      if (p.Cin % 32 == 0) disc_stage_halo_vec<DISC_WPITCH, DISC_WKC>(hl, p.x, ps, pt, plane, y0, x0, p.H, p.W, p.Cin, ci0);
      else disc_stage_halo<DISC_WPITCH>(hl, p.x, ps, pt, plane, y0, x0, p.H, p.W, p.Cin, ci0, kc);
    } else {
      disc3d_stage_halo_strided<S, AP>(hl, p.x, plane, y0, x0, p.H, p.W, p.Cin, kc);
    }
    if (p.Cout % 32 == 0) {
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int idx = threadIdx.x + it * 256, c4 = idx & 7, pix = idx >> 3;
        const int y = y0 + (pix >> 4), xx = x0 + (pix & 15);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (y < p.Ho && xx < p.Wo)
          v = *reinterpret_cast<const f32x4*>(p.dy + (((size_t)plane_o * p.Ho + y) * p.Wo + xx) * p.Cout + co0 + 4 * c4);
        *reinterpret_cast<f32x4*>(dyl + 4 * idx) = v;
      }
    } else {
      for (int idx = threadIdx.x; idx < 256 * 32; idx += 256) {
        const int co = idx & 31, pix = idx >> 5;
        const int y = y0 + (pix >> 4), xx = x0 + (pix & 15);
        float v = 0.f;
        if (y < p.Ho && xx < p.Wo && co0 + co < p.Cout) v = p.dy[(((size_t)plane_o * p.Ho + y) * p.Wo + xx) * p.Cout + co0 + co];
        dyl[idx] = v;
      }
    }
    __syncthreads();
    for (int s = 0; s < 32; ++s) {
      const int pi = 2 * s + kh, prow = 4 * wave + (pi >> 4), pcol = pi & 15;
      const float b = dyl[(prow * 16 + pcol) * 32 + j];
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) {
        const int ky = tp / 3, kx = tp % 3;
        const float a = j < kc ? hl[((prow * S + ky) * HS + pcol * S + kx) * AP + j] : 0.f;
        acc[tp] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[tp], 0, 0, 0);
      }
    }
    if (bias_wg) {
      const int co = threadIdx.x & 31, q = threadIdx.x >> 5;
      for (int k = 0; k < 32; ++k) bsum += dyl[(q * 32 + k) * 32 + co];
    }
  }

  // the four waves' accumulators, wave 0 first
  __syncthreads();
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int tp = 0; tp < 9; ++tp)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int idx = tp * 1024 + mfma_row(r, lane) * 32 + j;
          hl[idx] = w == 0 ? acc[tp][r] : hl[idx] + acc[tp][r];
        }
    }
    __syncthreads();
  }
  float* slab = p.slab + (size_t)blockIdx.x * p.slab_size;
  for (int idx = threadIdx.x; idx < 9 * 1024; idx += 256) {
    const int co = idx & 31, ci = (idx >> 5) & 31, tp = idx >> 10;
    if (ci0 + ci < p.Cin && co0 + co < p.Cout) slab[((size_t)(kt * 9 + tp) * p.Cin + ci0 + ci) * p.Cout + co0 + co] = hl[idx];
  }
  if (bias_wg) {
    dyl[threadIdx.x] = bsum;                                     // [q][co]
    __syncthreads();
    if (threadIdx.x < 32 && co0 + threadIdx.x < p.Cout) {
      float s = 0.f;
      for (int q = 0; q < 8; ++q) s += dyl[q * 32 + threadIdx.x];
      slab[(size_t)27 * p.Cin * p.Cout + co0 + threadIdx.x] = s;
    }
  }
}
