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
// The encoder's stage is a sibling kernel over the same parts (vae_wide_down_kernel, below):
//   down       'b c (t tc) (h hc) (w wc) -> b (tc hc wc c) t h w', the compression 1x1 conv K = Cin tc sc^2 -> Cout + the channel-area
//              residual of the rearranged input; M = a 16x16 tile of OUTPUT pixels, K walked as sub-position, chunk, channel pair.
//
// Every output is summed in the order time tap, channel chunk, spatial tap, channel pair, then the bias (and the residual); it
// depends on neither T, nor B, nor where a sequence was cut: a decode in chunks through the cache is bit-identical to the whole.
#pragma once
#include "disc_conv3.h"

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

// The store loops of VW_UP and VW_OUT for the accumulators of tile (y0, x0) of plane pl = n T + tau, sub-position `sub`, output
// channels n0 .. n0 + 32 NB - 1: + bias, then `up`'s rearranged position, or `out`'s area residual (read from p.x), split and
// frames.  Shared with the bf16-operand kernel of csrc/vae_wide_bf16.h, whose accumulators have the same layout.
template <int NB, int MODE>
__device__ __forceinline__ void vae_wide_store(const f32x16 (&acc)[2][NB], const VaeWideParams& p, int pl, int n, int tau, int sub,
                                               int n0, int y0, int x0) {
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
  vae_wide_store<NB, MODE>(acc, p, pl, n, tau, sub, n0, y0, x0);
}

// ---- down (reference: edm2/vae/vae.py :109-122, :136-141, :157-161).  Output pixel (t, y, x) at sub-position pos = (tq sc + hq) sc +
// wq reads input pixel (t tc + tq, y sc + hq, x sc + wq); the rearranged channel is k = pos Cin + c.  The input is fp32 or uint8
// addressed through element strides (b, t, h, w, c), normalised on load as vae_load_in of csrc/vae_encoder.hip does it.  Weights
// w[pos][CinP][CP], bias [CP].  One MFMA tap (the centre one): only the 16x16 interior of the stage is filled and read.
// out = (conv + bias) + area / len, area = the window [floor(o K / Cout), ceil((o + 1) K / Cout)) of output channel o summed in
// ascending k (the association of vae_down_kernel), read again from the input (vae_wide_area).  Every sum runs in an order set by (Cin, tc, sc, Cout) alone.
struct VaeWideDownParams {
  const void* x; const float* w; const float* bias;
  float* out;
  long long sb, st, sh, sw, sc;
  int B, To, Ho, Wo, Cin, CinP, Cout, CP, nblk, tiles_x, tiles_y, tc, scm, normalize;
};

template <typename TIN>
__device__ __forceinline__ float vae_wide_load_in(const TIN* p, int normalize) {
  const float v = (float)*p;
  return normalize ? __fsub_rn(__fdiv_rn(v, 127.5f), 1.f) : v;
}

// Channels c0 .. c0 + kc - 1 of the tile's 256 input pixels at one sub-position (xs: the sample's plane t tc + tq moved by hq rows
// and wq columns; ysh / xsw: the strides of one OUTPUT row / column) into the interior of hl; channels >= Cin and pixels outside
// the output plane are 0.  PITCH: the stage's pixel pitch (the weight gradient of csrc/vae_wide_train.hip stages 32 channels at 33).
template <typename TIN, int PITCH = DISC_APITCH>
__device__ __forceinline__ void vae_wide_stage_down(float* hl, const TIN* xs, long long ysh, long long xsw, long long sc, int normalize,
                                                    int y0, int x0, int Ho, int Wo, int Cin, int c0, int kc) {
  for (int idx = threadIdx.x; idx < DISC_TILE * DISC_TILE * kc; idx += 256) {
    const int c = idx % kc, pix = idx / kc, py = pix >> 4, px = pix & 15;
    const int y = y0 + py, xx = x0 + px;
    float v = 0.f;
    if (y < Ho && xx < Wo && c0 + c < Cin) v = vae_wide_load_in(xs + y * ysh + xx * xsw + (c0 + c) * sc, normalize);
    hl[((py + 1) * DISC_HALO + px + 1) * PITCH + c] = v;
  }
}

// The same for a full chunk of DISC_KC channels of contiguous fp32 whose channel count is a multiple of 32: 16-byte loads, all of a
// thread's loads issued before the first is used (the pattern of disc_stage_halo_vec).  Bit for bit what the scalar routine stores.
__device__ __forceinline__ void vae_wide_stage_down_vec(float* hl, const float* xs, long long ysh, long long xsw, int y0, int x0, int Ho,
                                                        int Wo, int c0) {
  constexpr int Q = DISC_KC / 4, IT = DISC_TILE * DISC_TILE * Q / 256;
  f32x4 v[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int idx = threadIdx.x + it * 256, q = idx % Q, pix = idx / Q;
    const int y = y0 + (pix >> 4), xx = x0 + (pix & 15);
    v[it] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (y < Ho && xx < Wo) v[it] = *reinterpret_cast<const f32x4*>(xs + y * ysh + xx * xsw + c0 + 4 * q);
  }
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int idx = threadIdx.x + it * 256, q = idx % Q, pix = idx / Q;
    float* o = hl + (((pix >> 4) + 1) * DISC_HALO + (pix & 15) + 1) * DISC_APITCH + 4 * q;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = v[it][e];
  }
}

// The window [s0, s1) of the rearranged channel axis at one output pixel (xp: the pixel's sub-position 0), summed in ascending k.
// Loads run ahead of the adds, eight values (VEC: four 16-byte loads) at a time; the adds keep their order.
template <typename TIN, bool VEC>
__device__ __forceinline__ float vae_wide_area(const TIN* xp, int s0, int s1, const VaeWideDownParams& p) {
  float area = 0.f;
  int pos = s0 / p.Cin, c = s0 - pos * p.Cin;
  for (int k = s0; k < s1; ++pos) {
    const TIN* xq = xp + (pos / (p.scm * p.scm)) * p.st + ((pos / p.scm) % p.scm) * p.sh + (pos % p.scm) * p.sw;
    const int ce = min(p.Cin, c + (s1 - k));
    k += ce - c;
    if (VEC) {
      const float* xf = (const float*)xq;
      for (; c < ce && (c & 3); ++c) area += xf[c];
      for (; c + 16 <= ce; c += 16) {
        f32x4 v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = *reinterpret_cast<const f32x4*>(xf + c + 4 * e);
#pragma unroll
        for (int e = 0; e < 16; ++e) area += v[e >> 2][e & 3];
      }
      for (; c + 4 <= ce; c += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xf + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) area += v[e];
      }
    }
    for (; c + 8 <= ce; c += 8) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = vae_wide_load_in(xq + (c + e) * p.sc, p.normalize);
#pragma unroll
      for (int e = 0; e < 8; ++e) area += v[e];
    }
    for (; c < ce; ++c) area += vae_wide_load_in(xq + c * p.sc, p.normalize);
    c = 0;
  }
  return area;
}

// The epilogue of `down` for the accumulators of tile (y0, x0) of output plane pl, output channels n0 .. n0 + 32 NB - 1 (xn: the
// sample's input at plane t tc): + bias + the area residual.  lds: the workgroup's LDS, [16][256] floats of it, free after the
// barrier this begins with.  Shared with the bf16-operand kernel of csrc/vae_wide_bf16.h.
template <int NB, typename TIN, bool VEC, bool RES>
__device__ __forceinline__ void vae_wide_down_store(const f32x16 (&acc)[2][NB], const VaeWideDownParams& p, float* lds, const TIN* xn,
                                                    int pl, int n0, int y0, int x0, long long ysh, long long xsw) {
  // the area residual: per lane the window of its output channel at its 32 pixels, each summed in ascending k; a rolled loop per
  // 16 pixels leaves the sums in the lane's own slots of the (now free) stage, and the unrolled store loop picks them up
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31;
  const long long K = (long long)(p.tc * p.scm * p.scm) * p.Cin;
  float* al = lds;                                               // [16][256]
  __syncthreads();
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int co = n0 + nb * 32 + j;
    if (co >= p.Cout) continue;
    const float bv = p.bias[co];
    const int s0 = (int)((co * K) / p.Cout), s1 = (int)(((co + 1) * K + p.Cout - 1) / p.Cout);
    const float len = (float)(s1 - s0);
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
#pragma unroll 1
      for (int r = 0; r < 16; ++r) {
        const int i = mfma_row(r, lane);
        const int y = y0 + 4 * wave + 2 * mb + (i >> 4), xx = x0 + (i & 15);
        float area = 0.f;
        if (RES && y < p.Ho && xx < p.Wo) area = vae_wide_area<TIN, VEC>(xn + y * ysh + xx * xsw, s0, s1, p);
        al[r * 256 + threadIdx.x] = area;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = mfma_row(r, lane);
        const int y = y0 + 4 * wave + 2 * mb + (i >> 4), xx = x0 + (i & 15);
        if (y >= p.Ho || xx >= p.Wo) continue;
        const float v = acc[mb][nb][r] + bv;
        p.out[(((size_t)pl * p.Ho + y) * p.Wo + xx) * p.Cout + co] = RES ? v + al[r * 256 + threadIdx.x] / len : v;
      }
    }
  }
}

// RES = false: out = conv + bias alone, the adjoint of `up` (csrc/vae_wide_train.hip: the sub-positions of d up gathered through W^T).
template <int NB, typename TIN, bool VEC, bool RES = true>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void vae_wide_down_kernel(VaeWideDownParams p) {
  extern __shared__ __attribute__((aligned(16))) float disc_lds[];
  float* hl = disc_lds;                                          // [324][17], the interior only
  float* wl = disc_lds + DISC_HALO * DISC_HALO * DISC_APITCH;    // [1][16][WP]
  const int tiles = p.tiles_x * p.tiles_y;
  const int tile = blockIdx.x % tiles, pl = blockIdx.x / tiles;  // pl = n To + t
  const int y0 = (tile / p.tiles_x) * DISC_TILE, x0 = (tile % p.tiles_x) * DISC_TILE;
  const int n0 = blockIdx.y * 32 * NB;
  const int n = pl / p.To, t = pl % p.To;
  const int P = p.tc * p.scm * p.scm;
  const long long ysh = p.scm * p.sh, xsw = p.scm * p.sw;
  const TIN* xn = (const TIN*)p.x + n * p.sb + (long long)t * p.tc * p.st;

  f32x16 acc[2][NB];
  disc_zero(acc);
  for (int pos = 0; pos < P; ++pos) {
    const TIN* xs = xn + (pos / (p.scm * p.scm)) * p.st + ((pos / p.scm) % p.scm) * p.sh + (pos % p.scm) * p.sw;
    for (int c0 = 0; c0 < p.CinP; c0 += DISC_KC) {
      const int kc = min(DISC_KC, p.CinP - c0);
      __syncthreads();
      if (VEC) vae_wide_stage_down_vec(hl, (const float*)xs, ysh, xsw, y0, x0, p.Ho, p.Wo, c0);
      else vae_wide_stage_down(hl, xs, ysh, xsw, p.sc, p.normalize, y0, x0, p.Ho, p.Wo, p.Cin, c0, kc);
      disc_stage_weights<NB>(wl, p.w, pos, 1, p.CinP, p.CP, c0, kc, n0);
      __syncthreads();
      vae_wide_mfma_taps<NB, 1>(acc, hl, wl, kc);
    }
  }
  vae_wide_down_store<NB, TIN, VEC, RES>(acc, p, disc_lds, xn, pl, n0, y0, x0, ysh, xsw);
}

// ---- host side (csrc/vae_wide.hip, csrc/vae_wide_train.hip)
static inline bool vae_wide_c_ok(int c) { return c > 0 && c <= 65536; }
static inline int vae_wide_nb(int CP) { return CP % 64 == 0 ? 2 : 1; }
// Conv A (and its data gradient, the same launch) of a block wider than 256 channels whose CP is a multiple of 128: 128 output
// channels per workgroup (NB = 4: the halo is staged half as often, 112 KB of LDS, one workgroup per CU), unless
// oniris_vae_wide_set_nb_max says 2.  The K loop is the same, so the bits are those of NB = 2.  No block of up to 256 channels gets here.
int oniris_vae_wide_nb_max(void);                                // csrc/misc.cpp
static inline int vae_wide_nb_conv_a(int C, int CP) {
  return C > 256 && CP % 128 == 0 && oniris_vae_wide_nb_max() >= 4 ? 4 : vae_wide_nb(CP);
}

template <int NB, int MODE>
static int vae_wide_launch(const char* what, const VaeWideParams& p, dim3 grid, hipStream_t stream) {
  constexpr int WP = (NB & 1) ? 32 * NB : 32 * NB + 32, TAPS = MODE == VW_CONV_A ? 9 : 1;
  const size_t bytes = ((size_t)DISC_HALO * DISC_HALO * DISC_APITCH + (size_t)TAPS * DISC_KC * WP) * sizeof(float);
  if (int rc = disc_raise_lds(vae_wide_kernel<NB, MODE>, bytes, what)) return rc;
  ONIRIS_KLAUNCH((vae_wide_kernel<NB, MODE>), grid, dim3(256), bytes, stream, p);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

// planes: the output planes a workgroup column walks; p.nsub, p.Cin, p.Cout, p.H, p.W set
template <int MODE>
static int vae_wide_dispatch(const char* what, VaeWideParams& p, long long planes, hipStream_t stream) {
  p.CinP = roundup(p.Cin, 2);
  p.CP = roundup(p.Cout, 32);
  p.tiles_x = cdiv(p.W, DISC_TILE); p.tiles_y = cdiv(p.H, DISC_TILE);
  const int nb = MODE == VW_CONV_A ? vae_wide_nb_conv_a(p.Cout, p.CP) : vae_wide_nb(p.CP);
  p.nblk = p.CP / (32 * nb);
  const long long wgs = planes * p.tiles_x * p.tiles_y;
  ONIRIS_CHECK_ARG(wgs <= 0x7fffffffLL && (long long)p.nsub * p.nblk <= 65535, "%s: %lld tiles", what, wgs);
  const dim3 grid((unsigned)wgs, p.nsub * p.nblk);
  if constexpr (MODE == VW_CONV_A)
    if (nb == 4) return vae_wide_launch<4, MODE>(what, p, grid, stream);
  return nb == 2 ? vae_wide_launch<2, MODE>(what, p, grid, stream) : vae_wide_launch<1, MODE>(what, p, grid, stream);
}

template <int NB, typename TIN, bool VEC, bool RES>
static int vae_wide_down_launch(const char* what, const VaeWideDownParams& p, dim3 grid, hipStream_t stream) {
  constexpr int WP = NB == 2 ? 96 : 32;
  const size_t bytes = ((size_t)DISC_HALO * DISC_HALO * DISC_APITCH + (size_t)DISC_KC * WP) * sizeof(float);
  if (int rc = disc_raise_lds(vae_wide_down_kernel<NB, TIN, VEC, RES>, bytes, what)) return rc;
  ONIRIS_KLAUNCH((vae_wide_down_kernel<NB, TIN, VEC, RES>), grid, dim3(256), bytes, stream, p);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

template <int NB, bool RES>
static int vae_wide_down_pick(const char* what, const VaeWideDownParams& p, int x_is_u8, bool vec, dim3 grid, hipStream_t stream) {
  if (RES && x_is_u8) return vae_wide_down_launch<NB, unsigned char, false, RES>(what, p, grid, stream);
  return vec ? vae_wide_down_launch<NB, float, true, RES>(what, p, grid, stream)
             : vae_wide_down_launch<NB, float, false, RES>(what, p, grid, stream);
}

// p: the operands, strides and sizes set; RES = false takes fp32 only
template <bool RES>
static int vae_wide_down_run(const char* what, VaeWideDownParams& p, int x_is_u8, hipStream_t stream) {
  p.CinP = roundup(p.Cin, 2);
  p.CP = roundup(p.Cout, 32);
  p.tiles_x = cdiv(p.Wo, DISC_TILE); p.tiles_y = cdiv(p.Ho, DISC_TILE);
  const int nb = vae_wide_nb(p.CP);
  p.nblk = p.CP / (32 * nb);
  const long long wgs = (long long)p.B * p.To * p.tiles_x * p.tiles_y;
  ONIRIS_CHECK_ARG(wgs <= 0x7fffffffLL && p.nblk <= 65535, "%s: %lld tiles", what, wgs);
  const bool vec = !x_is_u8 && !p.normalize && p.sc == 1 && p.Cin % 32 == 0 && p.sb % 4 == 0 && p.st % 4 == 0 && p.sh % 4 == 0 &&
                   p.sw % 4 == 0 && ((uintptr_t)p.x & 15) == 0;
  const dim3 grid((unsigned)wgs, p.nblk);
  return nb == 2 ? vae_wide_down_pick<2, RES>(what, p, x_is_u8, vec, grid, stream)
                 : vae_wide_down_pick<1, RES>(what, p, x_is_u8, vec, grid, stream);
}

// The 3x3 conv of disc_conv_kernel at a wide VAE width over `planes` planes: out = (res +) (bias +) conv3x3(x), res and bias or NULL;
// w packed [9][CinP][CP].  Conv B of a ResBlock, and its data gradient on flipped, transposed weights.
template <int NB>
static int vae_wide_conv3_launch(const char* what, const DiscConvParams& p, dim3 grid, hipStream_t stream) {
  constexpr int WP = NB == 2 ? 96 : 32;
  const size_t bytes = ((size_t)DISC_HALO * DISC_HALO * DISC_APITCH + (size_t)p.taps * DISC_KC * WP) * sizeof(float);
  if (int rc = disc_raise_lds(disc_conv_kernel<NB>, bytes, what)) return rc;
  ONIRIS_KLAUNCH(disc_conv_kernel<NB>, grid, dim3(256), bytes, stream, p);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

static int vae_wide_conv3_run(const char* what, const float* x, const float* res, const float* w, const float* bias, float* out,
                              long long planes, int H, int W, int C, hipStream_t stream) {
  DiscConvParams p;
  p.x = x; p.w = w; p.bias = bias; p.pro_s = nullptr; p.pro_t = nullptr; p.res = res; p.out = out; p.part = nullptr;
  p.N = (int)planes; p.H = H; p.W = W; p.Cin = C; p.CinP = roundup(C, 2); p.Cout = C; p.CoutP = roundup(C, 32); p.taps = 9;
  p.tiles_x = cdiv(W, DISC_TILE); p.tiles_y = cdiv(H, DISC_TILE); p.res_scale = 1.f;
  const long long wgs = planes * p.tiles_x * p.tiles_y;
  ONIRIS_CHECK_ARG(planes <= 0x7fffffffLL && wgs <= 0x7fffffffLL, "%s: %lld tiles", what, wgs);
  const int nb = vae_wide_nb(p.CoutP);
  const dim3 grid((unsigned)wgs, p.CoutP / (32 * nb));
  return nb == 2 ? vae_wide_conv3_launch<2>(what, p, grid, stream) : vae_wide_conv3_launch<1>(what, p, grid, stream);
}
