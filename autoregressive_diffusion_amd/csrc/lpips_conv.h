// The stride-1 convolutions of the LPIPS AlexNet trunk (5x5 64 -> 192, 3x3 192 -> 384 -> 256 -> 256) and their data gradients as one
// fp32 implicit GEMM on v_mfma_f32_32x32x2_f32.  Channels-last fp32 [image][y][x][C]; channel counts are multiples of 32 (input) and
// 64 (output).
//
//   M = the output pixels FLATTENED over (image, y, x): a workgroup of 256 threads owns 256 consecutive pixels, whichever images they
//       belong to (the maps are 15 x 15 at 256 x 256 frames and 3 x 3 at 64 x 64: a per-image 16 x 16 tile would leave most MFMA rows
//       empty exactly where the FLOPs are).  Wave w owns rows 64 w .. 64 w + 63 = two 32-row blocks.
//   N = 64 output channels (two 32-column blocks), blockIdx.y.
//   K = taps x Cin, walked tap by tap in chunks of 32 channels.  One iteration stages A [256][32] (the tap's shifted pixel of every
//       row, 0 outside its image: an im2col gather, 16-byte loads) and B [32][64] into LDS: 33.8 KB (pitch 33: the 32 rows of an
//       MFMA operand fall on 32 banks) + 12 KB (pitch 96: the two half-waves on disjoint banks) = 46 KB, three workgroups per CU.
//       The loads of iteration i + 1 are issued into registers before the 64 MFMAs per wave of iteration i.
//
// TM = 64 is the same kernel for launches that would not fill the machine with 256-row tiles (conv3-5 at 64 x 64 frames are 3 x 3 maps:
// 64 images are 576 rows): 64 pixels per workgroup, wave w owns the 32 x 32 block (rows 32 (w & 1), columns 32 (w >> 1)), 21 KB of LDS.
// Four times the workgroups, each with a quarter of the MFMA chain; the same bits.
//
// An output element is one k-ordered fmaf chain (tap-major, channel-minor) whatever row of whatever tile it lands in: its bits do not
// depend on the batch around it.  Epilogues: LPIPS_EPI_FWD relu(acc + bias[co]); LPIPS_EPI_BWD (acc + add[o]) * (f[o] > 0), add and f
// each optional -- the data gradient on flipped, transposed weights, `add` the head's gradient for that feature map and `f` the saved
// feature map whose sign is the ReLU mask.
#pragma once
#include "common.h"

#define LPIPS_TM 256
#define LPIPS_TM_SMALL 64
#define LPIPS_KC 32
#define LPIPS_APITCH 33
#define LPIPS_WN 64
#define LPIPS_WP 96
#define LPIPS_EPI_FWD 0
#define LPIPS_EPI_BWD 1

struct LpipsConvParams {
  const float* x; const float* w; const float* bias; const float* add; const float* f; float* out;
  long long M;                 // images x H x W
  int H, W, Cin, Cout;
};

template <int KS, int EPI, int TM>
__global__ __launch_bounds__(256) void lpips_conv_kernel(LpipsConvParams p) {
  constexpr int PAD = KS / 2;
  constexpr bool SMALL = TM == LPIPS_TM_SMALL;
  constexpr int MB = SMALL ? 1 : 2, NB = SMALL ? 1 : 2, RI = TM / 32;       // MFMA blocks per wave; staging passes of 32 rows
  __shared__ __attribute__((aligned(16))) float al[TM * LPIPS_APITCH];
  __shared__ __attribute__((aligned(16))) float wl[LPIPS_KC * LPIPS_WP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, kh = lane >> 5;
  const long long m0 = (long long)blockIdx.x * TM;
  const int row0 = SMALL ? 32 * (wave & 1) : 64 * wave, col0 = SMALL ? 32 * (wave >> 1) : 0;
  const int n0 = blockIdx.y * LPIPS_WN;
  const int HW = p.H * p.W;

  // the rows this thread stages: (tid >> 3) + 32 i, 16-byte column tid & 7
  const int q = tid & 7, r0 = tid >> 3;
  int ry[RI], rx[RI];
#pragma unroll
  for (int i = 0; i < RI; ++i) {
    const long long m = m0 + r0 + 32 * i;
    if (m < p.M) {
      const int rem = (int)(m % HW);
      ry[i] = rem / p.W;
      rx[i] = rem - ry[i] * p.W;
    } else {
      ry[i] = -(1 << 20);       // no tap of a row past the end is inside an image
      rx[i] = 0;
    }
  }
  const int bk = tid >> 4, bq = tid & 15;     // B: rows bk and bk + 16, 16-byte column bq

  f32x16 acc[MB][NB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;

  const int nchunk = p.Cin / LPIPS_KC, nit = KS * KS * nchunk;
  f32x4 av[RI], bv[2];

  auto fetch = [&](int it) {
    const int tap = it / nchunk, c0 = (it - tap * nchunk) * LPIPS_KC;
    const int dy = tap / KS - PAD, dx = tap % KS - PAD;
#pragma unroll
    for (int i = 0; i < RI; ++i) {
      const int y = ry[i] + dy, x = rx[i] + dx;
      av[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (y >= 0 && y < p.H && x >= 0 && x < p.W) {
        const long long src = m0 + r0 + 32 * i + dy * p.W + dx;
        av[i] = *reinterpret_cast<const f32x4*>(p.x + (size_t)src * p.Cin + c0 + 4 * q);
      }
    }
#pragma unroll
    for (int e = 0; e < 2; ++e)
      bv[e] = *reinterpret_cast<const f32x4*>(p.w + ((size_t)tap * p.Cin + c0 + bk + 16 * e) * p.Cout + n0 + 4 * bq);
  };

  fetch(0);
  for (int it = 0; it < nit; ++it) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RI; ++i) {
      float* o = al + (r0 + 32 * i) * LPIPS_APITCH + 4 * q;
      o[0] = av[i][0]; o[1] = av[i][1]; o[2] = av[i][2]; o[3] = av[i][3];
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) *reinterpret_cast<f32x4*>(wl + (bk + 16 * e) * LPIPS_WP + 4 * bq) = bv[e];
    __syncthreads();
    if (it + 1 < nit) fetch(it + 1);
    const float* ap = al + (row0 + j) * LPIPS_APITCH + kh;
    const float* bp = wl + kh * LPIPS_WP + col0 + j;
#pragma unroll 4
    for (int kk = 0; kk < LPIPS_KC; kk += 2) {
      float a[MB], b[NB];
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) a[mb] = ap[32 * mb * LPIPS_APITCH + kk];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) b[nb] = bp[kk * LPIPS_WP + 32 * nb];
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mb], b[nb], acc[mb][nb], 0, 0, 0);
    }
  }

#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int co = n0 + col0 + 32 * nb + j;
    const float bv0 = (EPI == LPIPS_EPI_FWD && p.bias) ? p.bias[co] : 0.f;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long long m = m0 + row0 + 32 * mb + mfma_row(r, lane);
        if (m >= p.M) continue;
        const size_t o = (size_t)m * p.Cout + co;
        float v = acc[mb][nb][r];
        if (EPI == LPIPS_EPI_FWD) {
          v = fmaxf(v + bv0, 0.f);
        } else {
          if (p.add) v += p.add[o];
          if (p.f) v = p.f[o] > 0.f ? v : 0.f;
        }
        p.out[o] = v;
      }
  }
}
