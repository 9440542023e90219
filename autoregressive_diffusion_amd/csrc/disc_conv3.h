// The 2-D discriminator's fp32 implicit-GEMM convolutions (reference: edm2/vae/discriminator.py, the nn.Conv2d of
// DiscriminatorBlock2D / Discriminator2D).  Channels-last fp32 [N][H][W][C]; one workgroup of 256 threads per 16x16 pixel tile of one
// image, the prologue vectors per channel.  The tile, the stages, the MFMA loops, the epilogue with its statistics and the slab
// store are csrc/disc_parts.h's, shared with csrc/disc_conv3d.h; here are the two kernels that walk them.
//
//   disc_conv_kernel<NB>   forward and data gradient, 3x3 (zero padding 1) or 1x1, 32 NB output channels per workgroup.
//   disc_wgrad_kernel<T>   weight and bias gradient of T taps: workgroup s walks the work items (image, tile) s, s + nslab, ... in
//                          that order and writes slab s.
#pragma once
#include "disc_parts.h"

struct DiscConvParams {
  const float* x; const float* w; const float* bias; const float* pro_s; const float* pro_t; const float* res;
  float* out; float* part;
  int N, H, W, Cin, CinP, Cout, CoutP, taps, tiles_x, tiles_y;
  float res_scale;
};

template <int NB>
__global__ __launch_bounds__(256) void disc_conv_kernel(DiscConvParams p) {
  extern __shared__ __attribute__((aligned(16))) float disc_lds[];
  float* hl = disc_lds;                                          // [324][17]
  float* wl = disc_lds + DISC_HALO * DISC_HALO * DISC_APITCH;    // [taps][16][WP]
  const int tile = blockIdx.x % (p.tiles_x * p.tiles_y), n = blockIdx.x / (p.tiles_x * p.tiles_y);
  const int y0 = (tile / p.tiles_x) * DISC_TILE, x0 = (tile % p.tiles_x) * DISC_TILE;
  const int n0 = blockIdx.y * 32 * NB;

  constexpr int WP = (NB & 1) ? 32 * NB : 32 * NB + 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, kh = lane >> 5;
  const int prow = 4 * wave + (j >> 4), pcol = j & 15;           // the lane's A pixel in row block 0; row block 1: prow + 2
  f32x16 acc[2][NB];
  disc_zero(acc);
  for (int c0 = 0; c0 < p.CinP; c0 += DISC_KC) {
    const int kc = min(DISC_KC, p.CinP - c0);
    __syncthreads();
    if (p.Cin % 32 == 0) disc_stage_halo_vec<DISC_APITCH, DISC_KC>(hl, p.x, p.pro_s, p.pro_t, n, y0, x0, p.H, p.W, p.Cin, c0);
    else disc_stage_halo<DISC_APITCH>(hl, p.x, p.pro_s, p.pro_t, n, y0, x0, p.H, p.W, p.Cin, c0, kc);
    disc_stage_weights<NB>(wl, p.w, 0, p.taps, p.CinP, p.CoutP, c0, kc, n0);
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
  disc_epilogue<NB>(acc, disc_lds, n, p.H, p.W, y0, x0, n0, p.Cout, p.bias, p.res, p.res_scale, p.out, p.part);
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
  const int ci0 = blockIdx.y * DISC_WKC, co0 = blockIdx.z * 32;
  const int kc = min(DISC_WKC, p.CinP - ci0);
  const int tiles = p.tiles_x * p.tiles_y;
  const bool bias_wg = blockIdx.y == 0;

  f32x16 acc[TAPS];
  disc_zero(acc);
  float bsum = 0.f;
  for (int item = blockIdx.x; item < p.nitems; item += p.nslab) {
    const int n = item / tiles, tile = item % tiles;
    const int y0 = (tile / p.tiles_x) * DISC_TILE, x0 = (tile % p.tiles_x) * DISC_TILE;
    __syncthreads();
    if (p.Cin % 32 == 0) disc_stage_halo_vec<DISC_WPITCH, DISC_WKC>(hl, p.x, p.pro_s, p.pro_t, n, y0, x0, p.H, p.W, p.Cin, ci0);
    else disc_stage_halo<DISC_WPITCH>(hl, p.x, p.pro_s, p.pro_t, n, y0, x0, p.H, p.W, p.Cin, ci0, kc);
    disc_stage_dy(dyl, p.dy, n, y0, x0, p.H, p.W, p.Cout, co0);
    __syncthreads();
    disc_wgrad_mfma<TAPS, 1, DISC_HALO, DISC_WPITCH>(acc, hl, dyl, kc);
    if (bias_wg) disc_bias_rows(bsum, dyl);
  }
  disc_wgrad_store<TAPS>(acc, bsum, hl, dyl, p.slab + (size_t)blockIdx.x * p.slab_size, 0, TAPS, bias_wg, p.Cin, p.Cout, ci0, co0);
}
