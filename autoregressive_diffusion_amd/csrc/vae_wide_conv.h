// The wide VAE decoder's fp32 implicit-GEMM kernel (reference: edm2/vae/vae.py :18-133), for block widths above the 64 channels
// that csrc/vae_conv3.h keeps in registers.  Channels-last fp32 [B][T][H][W][C]; one workgroup of 256 threads per 16x16 pixel tile
// of one plane of one sample and one block of 32 NB output channels, on v_mfma_f32_32x32x2_f32 over the parts of csrc/disc_parts.h
// (the stage of 18 x 18 x 16 channels, the weight stage, the lane map and, for conv A, the epilogue).  The loop nest is that of
// disc3d_conv_kernel<NB, 1>: time tap, 16-channel chunk, spatial tap, channel pair; no prologue (the operands arrive activated).
//
//   VW_CONV_A  the group-causal (2g, 3, 3) conv of a ResBlock on the sequence S = [B][g + T][H][W][C] (g prefix frames ++ T frames):
//              output frame tau g + gl reads planes tau g + kt, kt < 2g; out = bias + conv, raw.
//   VW_UP      the decompression 1x1 conv C -> C tc sc^2 stored at its 'b (tc hc wc c) t h w -> b c (t tc) (h hc) (w wc)' position.
//   VW_OUT     the final 1x1 conv Cin -> Cout + the channel-area residual; after the last block the mean | logvar split,
//              exp(logvar_multiplier) and the uint8 frames.
// The packed output channels are [nsub][CP] (CP = the width rounded up to a multiple of 32): sub = gl for conv A, (tq, hq, wq) for
// up, 0 for out, so that a block of output channels lies inside one output frame / sub-position and a lane's stores are
// contiguous over the channels.  Weights w[tap][CinP][nsub CP], CinP = Cin rounded up to even, zero where padded.
//
// Every output is summed in the order time tap, channel chunk, spatial tap, channel pair, then the bias (and the residual); it
// depends on neither T, nor B, nor where a sequence was cut: a decode in chunks through the cache is bit-identical to the whole.
#pragma once
#include "disc_parts.h"

enum { VW_CONV_A = 0, VW_UP = 1, VW_OUT = 2 };

struct VaeWideParams {
  const float* x; const float* w; const float* bias;
  float* out;
  int B, T, H, W, Cin, CinP, Cout, CP, nsub, nblk, g, tiles_x, tiles_y;
  int tc, sc;                                                    // VW_UP
  int split;                                                     // VW_OUT
  const float* lvm; float* out2; unsigned char* frames;
  long long sb, st, sh, sw, scs;
};

// TAPS = 9, or 1 = the centre tap, of one staged chunk: acc += A(tile pixels x kc channels) B(kc channels x 32 NB outputs)
template <int NB, int TAPS>
__device__ __forceinline__ void vae_wide_mfma_taps(f32x16 (&acc)[2][NB], const float* hl, const float* wl, int kc) {
  constexpr int WP = (NB & 1) ? 32 * NB : 32 * NB + 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, kh = lane >> 5;
  const int prow = 4 * wave + (j >> 4), pcol = j & 15;           // the lane's A pixel in row block 0; row block 1: prow + 2
  for (int tp = 0; tp < TAPS; ++tp) {
    const int ky = TAPS == 9 ? tp / 3 : 1, kx = TAPS == 9 ? tp % 3 : 1;
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

template <int NB, int MODE>
__global__ __launch_bounds__(256) void vae_wide_kernel(VaeWideParams p) {
  constexpr int TAPS = MODE == VW_CONV_A ? 9 : 1;
  extern __shared__ __attribute__((aligned(16))) float disc_lds[];
  float* hl = disc_lds;                                          // [324][17]
  float* wl = disc_lds + DISC_HALO * DISC_HALO * DISC_APITCH;    // [TAPS][16][WP]
  const int tiles = p.tiles_x * p.tiles_y;
  const int tile = blockIdx.x % tiles, pl = blockIdx.x / tiles;  // conv A: pl = n (T / g) + tau; else pl = n T + t
  const int y0 = (tile / p.tiles_x) * DISC_TILE, x0 = (tile % p.tiles_x) * DISC_TILE;
  const int sub = blockIdx.y / p.nblk, n0 = (blockIdx.y % p.nblk) * 32 * NB;
  const int CoutP = p.nsub * p.CP;
  const int ntau = MODE == VW_CONV_A ? p.T / p.g : 1;
  const int n = MODE == VW_CONV_A ? pl / ntau : pl / p.T;
  const int tau = MODE == VW_CONV_A ? pl % ntau : pl % p.T;
  const int KT = MODE == VW_CONV_A ? 2 * p.g : 1;
  const int plane0 = MODE == VW_CONV_A ? n * (p.g + p.T) + tau * p.g : pl;

  f32x16 acc[2][NB];
  disc_zero(acc);
  for (int kt = 0; kt < KT; ++kt) {
    for (int c0 = 0; c0 < p.CinP; c0 += DISC_KC) {
      const int kc = min(DISC_KC, p.CinP - c0);
      __syncthreads();
      if (p.Cin % 32 == 0) disc_stage_halo_vec<DISC_APITCH, DISC_KC>(hl, p.x, nullptr, nullptr, plane0 + kt, y0, x0, p.H, p.W, p.Cin, c0);
      else disc_stage_halo<DISC_APITCH>(hl, p.x, nullptr, nullptr, plane0 + kt, y0, x0, p.H, p.W, p.Cin, c0, kc);
      disc_stage_weights<NB>(wl, p.w, kt * TAPS, TAPS, p.CinP, CoutP, c0, kc, sub * p.CP + n0);
      __syncthreads();
      vae_wide_mfma_taps<NB, TAPS>(acc, hl, wl, kc);
    }
  }

  if (MODE == VW_CONV_A) {
    disc_epilogue<NB>(acc, disc_lds, n * p.T + tau * p.g + sub, p.H, p.W, y0, x0, n0, p.Cout, p.bias + sub * p.CP, nullptr, 1.f, p.out,
                      nullptr);
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int co = n0 + nb * 32 + j;
    if (co >= p.Cout) continue;
    const float bv = p.bias[sub * p.CP + co];
    int s0 = 0, s1 = 1;
    float scale = 1.f;
    if (MODE == VW_OUT) {
      s0 = (co * p.Cin) / p.Cout;
      s1 = ((co + 1) * p.Cin + p.Cout - 1) / p.Cout;
      if (p.split > 0 && co >= p.split) scale = expf(*p.lvm);
    }
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = mfma_row(r, lane);
        const int y = y0 + 4 * wave + 2 * mb + (i >> 4), xx = x0 + (i & 15);
        if (y >= p.H || xx >= p.W) continue;
        float v = acc[mb][nb][r] + bv;
        if (MODE == VW_UP) {
          const int wq = sub % p.sc, hq = (sub / p.sc) % p.sc, tq = sub / (p.sc * p.sc);
          const size_t plane_o = (size_t)n * p.T * p.tc + (size_t)tau * p.tc + tq;
          p.out[((plane_o * (p.H * p.sc) + (size_t)y * p.sc + hq) * (p.W * p.sc) + (size_t)xx * p.sc + wq) * p.Cout + co] = v;
        } else {
          const size_t pix = ((size_t)pl * p.H + y) * p.W + xx;
          const float* xp = p.x + pix * p.Cin;
          float area = 0.f;
          for (int ci = s0; ci < s1; ++ci) area += xp[ci];
          v += area / (float)(s1 - s0);
          const long long o = (long long)n * p.sb + (long long)tau * p.st + (long long)y * p.sh + (long long)xx * p.sw;
          if (p.split > 0 && co >= p.split) {
            if (p.out) p.out2[o + (long long)(co - p.split) * p.scs] = v * scale;
            continue;
          }
          if (p.out) p.out[o + (long long)co * p.scs] = v;
          if (p.frames) {
            float f = (v + 1.f) * 127.5f;
            f = fminf(fmaxf(f, 0.f), 255.f);
            p.frames[pix * p.split + co] = (unsigned char)(int)f;
          }
        }
      }
  }
}
