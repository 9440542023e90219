// The 3-D discriminator's fp32 implicit-GEMM convolutions (reference: edm2/vae/discriminator.py, the nn.Conv3d of
// DiscriminatorBlock3D / Discriminator3D).  Channels-last fp32 [N][T][H][W][C]; a 27-tap conv is the sum over kt of three 9-tap
// convs of the planes t S + kt - 1, so these kernels walk the parts of csrc/disc_parts.h that the 2-D kernels (csrc/disc_conv3.h)
// walk, with one more loop level; planes outside 0 .. T - 1 are skipped.  One workgroup of 256 threads per 16x16 tile of one
// output plane of one sample: a tile never spans two samples, and the prologue vectors are per (sample, channel).
//
//   disc3d_conv_kernel<NB, S>   S = 1: forward and data gradient of the 27-tap convs, zero padding 1, operand staged by
//                               disc_stage_halo(_vec) -- LDS as the 2-D kernel's.  S = 2: the stem conv_in, stride 2 in T, H and W,
//                               1..8 input channels padded to 8: the stage is the 33 x 33 input positions a tile of outputs reads
//                               (pitch 9: 38 KB), output position (y, x) tap (ky, kx) reads stage position (2 y + ky, 2 x + kx).
//   disc3d_wgrad_kernel<S>      weight and bias gradient: blockIdx.y carries kt and the 32-channel block of Cin, so a workgroup
//                               holds the 9 accumulator blocks of one kt and pairs plane t S + kt - 1 of the operand with plane t of
//                               dy; workgroup s walks the work items (sample, plane, tile) s, s + nslab, ... and writes slab s.
#pragma once
#include "disc_parts.h"

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
  constexpr int HS = 15 * S + 3, AP = S == 1 ? DISC_APITCH : 9;
  extern __shared__ __attribute__((aligned(16))) float disc_lds[];
  float* hl = disc_lds;                                          // [HS * HS][AP]
  float* wl = disc_lds + HS * HS * AP;                           // [9][16][WP]
  const int tiles = p.tiles_x * p.tiles_y;
  const int tile = blockIdx.x % tiles, plane_o = blockIdx.x / tiles;             // plane_o = n To + to
  const int n = plane_o / p.To, to = plane_o % p.To;
  const int y0 = (tile / p.tiles_x) * DISC_TILE, x0 = (tile % p.tiles_x) * DISC_TILE;
  const int n0 = blockIdx.y * 32 * NB;
  const float* ps = p.pro_s ? p.pro_s + (size_t)n * p.Cin : nullptr;
  const float* pt = p.pro_t ? p.pro_t + (size_t)n * p.Cin : nullptr;

  constexpr int WP = (NB & 1) ? 32 * NB : 32 * NB + 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, kh = lane >> 5;
  const int prow = 4 * wave + (j >> 4), pcol = j & 15;           // the lane's A pixel in row block 0; row block 1: prow + 2
  f32x16 acc[2][NB];
  disc_zero(acc);
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
      disc_stage_weights<NB>(wl, p.w, kt * 9, 9, p.CinP, p.CoutP, c0, kc, n0);
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
  disc_epilogue<NB>(acc, disc_lds, plane_o, p.Ho, p.Wo, y0, x0, n0, p.Cout, p.bias, p.res, p.res_scale, p.out, p.part);
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
  const int kt = blockIdx.y / p.ncib, ci0 = (blockIdx.y % p.ncib) * DISC_WKC, co0 = blockIdx.z * 32;
  const int kc = min(DISC_WKC, p.CinP - ci0);
  const int tiles = p.tiles_x * p.tiles_y;
  const bool bias_wg = blockIdx.y == p.ncib;                     // kt = 1, the first channel block: its plane always exists

  f32x16 acc[9];
  disc_zero(acc);
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
    disc_stage_dy(dyl, p.dy, plane_o, y0, x0, p.Ho, p.Wo, p.Cout, co0);
    __syncthreads();
    disc_wgrad_mfma<9, S, HS, AP>(acc, hl, dyl, kc);
    if (bias_wg) disc_bias_rows(bsum, dyl);
  }
  disc_wgrad_store<9>(acc, bsum, hl, dyl, p.slab + (size_t)blockIdx.x * p.slab_size, kt * 9, 27, bias_wg, p.Cin, p.Cout, ci0, co0);
}
