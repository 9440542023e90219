// LPIPS (net = 'alex', weights layout 0.1): the perceptual loss of the VAE's training loop, forward and backward, fp32 throughout.
// include/oniris.h: oniris_lpips_*; autoregressive_diffusion_amd/lpips.py drives them.  Activations are channels-last [image][y][x][C];
// both operands go through the trunk as one batch of 2 N images (operand 0 first).
//
//   lpips_stem_kernel        (x - shift) / scale, the 11 x 11 stride-4 pad-2 conv 3 -> 64, bias and ReLU in one launch from the strided
//                            operands, on v_mfma_f32_32x32x2_f32.  A workgroup of 256 threads owns 8 x 16 output pixels and stages their
//                            39 x 71 x 3 scaled patch in LDS (35.6 KB), columns split by x mod 4 so that the 16 pixels of a tile row read
//                            consecutive words for every tap: the A operand is read straight from the patch, no im2col copy.  The
//                            weights pass LDS one kernel row at a time (36 x 64, 13.8 KB; kx padded to 12 with a zero row).
//   lpips_stem_dgrad_kernel  its data gradient, divided by scale, written with the strides of the operand's gradient.  A workgroup owns
//                            32 x 32 input pixels and stages the 11 x 11 x 64 gradients they draw from (pitch 68: 33 KB); wave w takes the
//                            pixels of phase (y mod 4, x mod 4) = w, w + 4, w + 8, w + 12, so the tap of every lane is the same and the
//                            weights are again wave-uniform.
//   lpips_conv_kernel        lpips_conv.h: the stride-1 convs and their data gradients.
//   lpips_pool_kernel        max-pool 3 x 3 stride 2, floor mode.
//   lpips_pool_bwd_kernel    its adjoint in gather form: an input position collects from the up to four windows it lies in and is the
//                            FIRST maximum of (row-major window order); optional + add and the ReLU mask of the pooled map.  No atomics.
//   lpips_head_fwd_kernel    per layer: one wave per pixel reads both operands' features, forms the two norms and the weighted squared
//                            difference; a workgroup sums its 64 pixels (wave w: pixels w, w + 4, ... in that order, then the four waves
//                            in order) into part [image][chunk].  lpips_head_sum_kernel adds the chunks and the layers in order.
//   lpips_head_bwd_kernel    per layer: d f for the operands that need it from the cotangent [N] on the device.
// A pixel whose channels are all 0 has the unit vector 0 and takes no gradient (torch's adjoint is 0 / 0 there).
// Every sum has a fixed order that does not depend on N; nothing synchronises with the host.
#include "oniris.h"
#include "common.h"
#include "lpips_conv.h"

#define LPIPS_EPS 1e-10f

// ------------------------------------------------------------------------------------------------------------------------------------
// stem

#define STEM_TY 8
#define STEM_TX 16
#define STEM_PH (4 * (STEM_TY - 1) + 11)      // 39
#define STEM_PW (4 * (STEM_TX - 1) + 11)      // 71
#define STEM_PWQ 19                           // > ceil(71 / 4); 48 x 19 = 16 mod 64: the four tile rows of a wave on disjoint banks

struct LpipsStrides { long long n, c, h, w; };

#define STEM_WK 36                            // K rows of one ky: 3 channels x 12 taps (kx = 11 is a zero row: K even for the MFMA)
#define STEM_WP 96                            // the two half-waves of a B read on disjoint banks

// wp [ky][c][kx][64].  M = the 128 pixels of the tile (wave w: tile rows 2 w, 2 w + 1), N = 64, K = 11 x 36 walked ky by ky.
__global__ __launch_bounds__(256) void lpips_stem_kernel(const float* __restrict__ in0, const float* __restrict__ in1, LpipsStrides s0,
                                                         LpipsStrides s1, int N, int H, int W, int H1, int W1, int normalize,
                                                         const float* __restrict__ shift, const float* __restrict__ scale,
                                                         const float* __restrict__ wp, const float* __restrict__ bias,
                                                         float* __restrict__ f1, int tiles_x, int tiles_y) {
  __shared__ float patch[STEM_PH * 3 * 4 * STEM_PWQ];
  __shared__ __attribute__((aligned(16))) float wl[STEM_WK * STEM_WP];
  const int tile = blockIdx.x % (tiles_x * tiles_y), n = blockIdx.x / (tiles_x * tiles_y);
  const int oy0 = (tile / tiles_x) * STEM_TY, ox0 = (tile % tiles_x) * STEM_TX;
  const float* src = n < N ? in0 : in1;
  const LpipsStrides s = n < N ? s0 : s1;
  const long long nb0 = (long long)(n < N ? n : n - N) * s.n;
  // columns 0 .. 71: column 71 is what the zero tap kx = 11 of the last tile column reads, and must be finite
  for (int idx = threadIdx.x; idx < STEM_PH * 3 * (STEM_PW + 1); idx += 256) {
    const int px = idx % (STEM_PW + 1), c = (idx / (STEM_PW + 1)) % 3, py = idx / (3 * (STEM_PW + 1));
    const int iy = 4 * oy0 - 2 + py, ix = 4 * ox0 - 2 + px;
    float v = 0.f;
    if (px < STEM_PW && iy >= 0 && iy < H && ix >= 0 && ix < W) {
      v = src[nb0 + c * s.c + iy * s.h + ix * s.w];
      if (normalize) v = 2.f * v - 1.f;
      v = (v - shift[c]) / scale[c];
    }
    patch[((py * 3 + c) * 4 + (px & 3)) * STEM_PWQ + (px >> 2)] = v;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, kh = lane >> 5;
  const int ty = 2 * wave + (j >> 4), tx = j & 15;
  f32x16 acc[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;
  for (int ky = 0; ky < 11; ++ky) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < STEM_WK * 16; idx += 256) {
      const int c4 = idx & 15, kx = (idx >> 4) % 12, c = idx / (16 * 12);
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (kx < 11) v = *reinterpret_cast<const f32x4*>(wp + (size_t)(((ky * 3 + c) * 11 + kx) * 64) + 4 * c4);
      *reinterpret_cast<f32x4*>(wl + (c * 12 + kx) * STEM_WP + 4 * c4) = v;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* prow = patch + ((4 * ty + ky) * 3 + c) * 4 * STEM_PWQ + tx;
#pragma unroll
      for (int st = 0; st < 6; ++st) {
        const int kx = 2 * st + kh;
        const float a = prow[(kx & 3) * STEM_PWQ + (kx >> 2)];
        const float* bp = wl + (c * 12 + kx) * STEM_WP + j;
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[0], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[32], acc[1], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    const float bv = bias[32 * nb + j];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = mfma_row(r, lane);
      const int oy = oy0 + 2 * wave + (i >> 4), ox = ox0 + (i & 15);
      if (oy < H1 && ox < W1) f1[(((size_t)n * H1 + oy) * W1 + ox) * 64 + 32 * nb + j] = fmaxf(acc[nb][r] + bv, 0.f);
    }
  }
}

#define SDG_T 32
#define SDG_G 11
#define SDG_PITCH 68

// g1 [NI][H1][W1][64] (already masked by the stem's ReLU); wd [ky][kx][c][64]; dx (NI, 3, H, W) by element strides
__global__ __launch_bounds__(256) void lpips_stem_dgrad_kernel(const float* __restrict__ g1, const float* __restrict__ wd,
                                                               const float* __restrict__ scale, int H, int W, int H1, int W1,
                                                               int normalize, float* __restrict__ dx, LpipsStrides ds, int tiles_x,
                                                               int tiles_y) {
  __shared__ __attribute__((aligned(16))) float gl[SDG_G * SDG_G * SDG_PITCH];
  const int tile = blockIdx.x % (tiles_x * tiles_y), n = blockIdx.x / (tiles_x * tiles_y);
  const int y0 = (tile / tiles_x) * SDG_T, x0 = (tile % tiles_x) * SDG_T;
  const int gy0 = y0 / 4 - 2, gx0 = x0 / 4 - 2;
  for (int idx = threadIdx.x; idx < SDG_G * SDG_G * 16; idx += 256) {
    const int c4 = idx & 15, pix = idx >> 4;
    const int oy = gy0 + pix / SDG_G, ox = gx0 + pix % SDG_G;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (oy >= 0 && oy < H1 && ox >= 0 && ox < W1) v = *reinterpret_cast<const f32x4*>(g1 + (((size_t)n * H1 + oy) * W1 + ox) * 64 + 4 * c4);
    *reinterpret_cast<f32x4*>(gl + pix * SDG_PITCH + 4 * c4) = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int by = lane >> 3, bx = lane & 7;
  // the four phases of this wave; the stores wait until every weight has been read (the loads of the weights stay scalar loads)
  float res[4][3];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ph = wave + 4 * i;
    const int ty = (ph >> 2) + 2, tx = (ph & 3) + 2;  // y + 2 = y0 + 4 by + ty: ky = (ty & 3) + 4 jy at output row y0 / 4 + by + (ty >> 2) - jy
    float acc[3] = {0.f, 0.f, 0.f};
    for (int jy = 0; jy < 3; ++jy) {
      const int ky = (ty & 3) + 4 * jy;
      if (ky > 10) break;
      const int ly = by + (ty >> 2) - jy + 2;
      for (int jx = 0; jx < 3; ++jx) {
        const int kx = (tx & 3) + 4 * jx;
        if (kx > 10) break;
        const int lx = bx + (tx >> 2) - jx + 2;
        const float* gp = gl + (ly * SDG_G + lx) * SDG_PITCH;
        const float* wr = wd + (size_t)((ky * 11 + kx) * 3) * 64;
#pragma unroll
        for (int c4 = 0; c4 < 16; ++c4) {
          const f32x4 g = *reinterpret_cast<const f32x4*>(gp + 4 * c4);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = __builtin_fmaf(g[e], wr[c * 64 + 4 * c4 + e], acc[c]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) res[i][c] = acc[c];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ph = wave + 4 * i;
    const int y = y0 + 4 * by + (ph >> 2), x = x0 + 4 * bx + (ph & 3);
    if (y < H && x < W) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float v = res[i][c] / scale[c];
        if (normalize) v = 2.f * v;
        dx[n * ds.n + c * ds.c + y * ds.h + x * ds.w] = v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// max-pool 3 x 3 stride 2

__global__ __launch_bounds__(256) void lpips_pool_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W, int Ho,
                                                         int Wo, int C4, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c4 = (int)(idx % C4);
  long long t = idx / C4;
  const int ox = (int)(t % Wo); t /= Wo;
  const int oy = (int)(t % Ho);
  const long long n = t / Ho;
  const f32x4* xp = reinterpret_cast<const f32x4*>(x) + ((n * H + 2 * oy) * W + 2 * ox) * C4 + c4;
  f32x4 m = xp[0];
#pragma unroll
  for (int wy = 0; wy < 3; ++wy)
#pragma unroll
    for (int wx = 0; wx < 3; ++wx) {
      const f32x4 v = xp[((long long)wy * W + wx) * C4];
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
    }
  reinterpret_cast<f32x4*>(out)[idx] = m;
}

__global__ __launch_bounds__(256) void lpips_pool_bwd_kernel(const float* __restrict__ dp, const float* __restrict__ f,
                                                             const float* add, int mask, float* out, int H, int W, int Ho,
                                                             int Wo, int C4, long long total) {      // out may be add
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c4 = (int)(idx % C4);
  long long t = idx / C4;
  const int x = (int)(t % W); t /= W;
  const int y = (int)(t % H);
  const long long n = t / H;
  const f32x4* fp = reinterpret_cast<const f32x4*>(f);
  const f32x4 val = fp[idx];
  f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f};
  const int oy_lo = y >= 1 ? (y - 1) >> 1 : 0, oy_hi = min(Ho - 1, y >> 1);
  const int ox_lo = x >= 1 ? (x - 1) >> 1 : 0, ox_hi = min(Wo - 1, x >> 1);
  for (int oy = oy_lo; oy <= oy_hi; ++oy)
    for (int ox = ox_lo; ox <= ox_hi; ++ox) {
      const int pidx = (y - 2 * oy) * 3 + (x - 2 * ox);
      bool first[4] = {true, true, true, true};
#pragma unroll
      for (int qi = 0; qi < 9; ++qi) {
        if (qi == pidx) continue;
        const f32x4 v = fp[((n * H + 2 * oy + qi / 3) * W + 2 * ox + qi % 3) * C4 + c4];
#pragma unroll
        for (int e = 0; e < 4; ++e) first[e] = first[e] && (qi < pidx ? val[e] > v[e] : val[e] >= v[e]);
      }
      const f32x4 d = reinterpret_cast<const f32x4*>(dp)[((n * Ho + oy) * Wo + ox) * C4 + c4];
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] += first[e] ? d[e] : 0.f;
    }
  if (add) {
    const f32x4 a = reinterpret_cast<const f32x4*>(add)[idx];
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] += a[e];
  }
  if (mask) {
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = val[e] > 0.f ? g[e] : 0.f;
  }
  reinterpret_cast<f32x4*>(out)[idx] = g;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// heads

#define HEAD_PIX 64
#define HEAD_CPL 6            // channels per lane: C <= 384

__device__ __forceinline__ float lpips_rnorm(float s) { return s > 0.f ? 1.f / (sqrtf(s) + LPIPS_EPS) : 0.f; }

__global__ __launch_bounds__(256) void lpips_head_fwd_kernel(const float* __restrict__ fa, const float* __restrict__ fb,
                                                             const float* __restrict__ w, float* __restrict__ part, int HW, int C, int P) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = blockIdx.y, cpl = C >> 6;
  float wv[HEAD_CPL];
#pragma unroll
  for (int i = 0; i < HEAD_CPL; ++i) wv[i] = i < cpl ? w[lane + 64 * i] : 0.f;
  float s = 0.f;
  for (int pi = wave; pi < HEAD_PIX; pi += 4) {
    const int pix = blockIdx.x * HEAD_PIX + pi;
    if (pix >= HW) break;
    const float* a = fa + ((size_t)n * HW + pix) * C + lane;
    const float* b = fb + ((size_t)n * HW + pix) * C + lane;
    float av[HEAD_CPL], bv[HEAD_CPL], sa = 0.f, sb = 0.f;
#pragma unroll
    for (int i = 0; i < HEAD_CPL; ++i) {
      av[i] = i < cpl ? a[64 * i] : 0.f;
      bv[i] = i < cpl ? b[64 * i] : 0.f;
      sa = __builtin_fmaf(av[i], av[i], sa);
      sb = __builtin_fmaf(bv[i], bv[i], sb);
    }
    const float ra = lpips_rnorm(wave_sum(sa)), rb = lpips_rnorm(wave_sum(sb));
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < HEAD_CPL; ++i) {
      const float d = av[i] * ra - bv[i] * rb;
      t = __builtin_fmaf(wv[i] * d, d, t);
    }
    s += wave_sum(t);
  }
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)n * P + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

struct LpipsHeadSumParams { long long off[8]; int P[8]; int HW[8]; int layers; };

__global__ void lpips_head_sum_kernel(const float* __restrict__ part, LpipsHeadSumParams p, int N, float* __restrict__ out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float total = 0.f;
  for (int k = 0; k < p.layers; ++k) {
    const float* q = part + p.off[k] + (size_t)n * p.P[k];
    float s = 0.f;
    for (int i = 0; i < p.P[k]; ++i) s += q[i];
    total += s / (float)p.HW[k];
  }
  out[n] = total;
}

__global__ __launch_bounds__(256) void lpips_head_bwd_kernel(const float* __restrict__ fa, const float* __restrict__ fb,
                                                             const float* __restrict__ w, const float* __restrict__ cot,
                                                             float* __restrict__ ga, float* __restrict__ gb, int mask, int HW, int C) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = blockIdx.y, cpl = C >> 6;
  const float coef = 2.f * (cot[n] / (float)HW);
  float wv[HEAD_CPL];
#pragma unroll
  for (int i = 0; i < HEAD_CPL; ++i) wv[i] = i < cpl ? w[lane + 64 * i] : 0.f;
  for (int pi = wave; pi < HEAD_PIX; pi += 4) {
    const int pix = blockIdx.x * HEAD_PIX + pi;
    if (pix >= HW) break;
    const size_t base = ((size_t)n * HW + pix) * C + lane;
    float av[HEAD_CPL], bv[HEAD_CPL], ev[HEAD_CPL], sa = 0.f, sb = 0.f;
#pragma unroll
    for (int i = 0; i < HEAD_CPL; ++i) {
      av[i] = i < cpl ? fa[base + 64 * i] : 0.f;
      bv[i] = i < cpl ? fb[base + 64 * i] : 0.f;
      sa = __builtin_fmaf(av[i], av[i], sa);
      sb = __builtin_fmaf(bv[i], bv[i], sb);
    }
    sa = wave_sum(sa);
    sb = wave_sum(sb);
    const float ra = lpips_rnorm(sa), rb = lpips_rnorm(sb);
    float da = 0.f, db = 0.f;
#pragma unroll
    for (int i = 0; i < HEAD_CPL; ++i) {
      const float d = av[i] * ra - bv[i] * rb;
      ev[i] = coef * (wv[i] * d);
      da = __builtin_fmaf(ev[i], av[i], da);
      db = __builtin_fmaf(ev[i], bv[i], db);
    }
    da = wave_sum(da);
    db = wave_sum(db);
    // d u / d a = 1 / (|a| + eps) - a a^T / (|a| (|a| + eps)^2); a pixel of zeros takes no gradient
    const float ka = sa > 0.f ? da * ra * ra / sqrtf(sa) : 0.f;
    const float kb = sb > 0.f ? db * rb * rb / sqrtf(sb) : 0.f;
#pragma unroll
    for (int i = 0; i < HEAD_CPL; ++i) {
      if (i >= cpl) break;
      if (ga) {
        float v = ev[i] * ra - av[i] * ka;
        if (mask) v = av[i] > 0.f ? v : 0.f;
        ga[base + 64 * i] = v;
      }
      if (gb) {
        float v = bv[i] * kb - ev[i] * rb;
        if (mask) v = bv[i] > 0.f ? v : 0.f;
        gb[base + 64 * i] = v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// C ABI

static inline LpipsStrides lpips_strides(const long long* s) { return LpipsStrides{s[0], s[1], s[2], s[3]}; }

extern "C" int oniris_lpips_stem(const float* in0, const float* in1, const long long* stride0, const long long* stride1, int N, int H,
                                 int W, int normalize, const float* shift, const float* scale, const float* wp, const float* bias,
                                 float* f1, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(in0 && in1 && stride0 && stride1 && shift && scale && wp && bias && f1 && N > 0, "lpips_stem: bad arguments");
  ONIRIS_CHECK_ARG(H >= 11 - 4 && W >= 11 - 4, "lpips_stem: %d x %d is smaller than the kernel", H, W);
  const int H1 = (H + 4 - 11) / 4 + 1, W1 = (W + 4 - 11) / 4 + 1;
  const int tx = cdiv(W1, STEM_TX), ty = cdiv(H1, STEM_TY);
  const long long wgs = 2LL * N * tx * ty;
  ONIRIS_CHECK_ARG(wgs <= 0x7fffffffLL, "lpips_stem: %lld tiles", wgs);
  ONIRIS_KLAUNCH(lpips_stem_kernel, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, in0, in1, lpips_strides(stride0),
                 lpips_strides(stride1), N, H, W, H1, W1, normalize, shift, scale, wp, bias, f1, tx, ty);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_lpips_stem_dgrad(const float* g1, const float* wd, const float* scale, int NI, int H, int W, int normalize,
                                       float* dx, const long long* dstride, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(g1 && wd && scale && dx && dstride && NI > 0 && H >= 7 && W >= 7, "lpips_stem_dgrad: bad arguments");
  const int H1 = (H + 4 - 11) / 4 + 1, W1 = (W + 4 - 11) / 4 + 1;
  const int tx = cdiv(W, SDG_T), ty = cdiv(H, SDG_T);
  const long long wgs = (long long)NI * tx * ty;
  ONIRIS_CHECK_ARG(wgs <= 0x7fffffffLL, "lpips_stem_dgrad: %lld tiles", wgs);
  ONIRIS_KLAUNCH(lpips_stem_dgrad_kernel, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, g1, wd, scale, H, W, H1, W1, normalize,
                 dx, lpips_strides(dstride), tx, ty);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

template <int KS, int EPI>
static void lpips_conv_launch(const LpipsConvParams& p, int tile, hipStream_t stream) {
  const dim3 grid((unsigned)((p.M + tile - 1) / tile), p.Cout / LPIPS_WN);
  if (tile == LPIPS_TM_SMALL) ONIRIS_KLAUNCH((lpips_conv_kernel<KS, EPI, LPIPS_TM_SMALL>), grid, dim3(256), 0, stream, p);
  else ONIRIS_KLAUNCH((lpips_conv_kernel<KS, EPI, LPIPS_TM>), grid, dim3(256), 0, stream, p);
}

extern "C" int oniris_lpips_conv(const float* x, const float* wp, const float* bias, const float* add, const float* f, float* out,
                                 long long NI, int H, int W, int Cin, int Cout, int ksize, int mode, int tile,
                                 oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && wp && out && NI > 0 && H > 0 && W > 0, "lpips_conv: bad arguments");
  ONIRIS_CHECK_ARG(ksize == 3 || ksize == 5, "lpips_conv: kernel size %d (3 or 5)", ksize);
  ONIRIS_CHECK_ARG(mode == LPIPS_EPI_FWD || mode == LPIPS_EPI_BWD, "lpips_conv: mode %d", mode);
  ONIRIS_CHECK_ARG(tile == 0 || tile == LPIPS_TM || tile == LPIPS_TM_SMALL, "lpips_conv: tile %d (0, 64 or 256)", tile);
  ONIRIS_CHECK_ARG(Cin > 0 && Cin % LPIPS_KC == 0 && Cout > 0 && Cout % LPIPS_WN == 0,
                   "lpips_conv: Cin %d must be a multiple of 32 and Cout %d of 64", Cin, Cout);
  ONIRIS_CHECK_ARG(mode == LPIPS_EPI_FWD ? (bias && !add && !f) : !bias, "lpips_conv: forward takes a bias, the gradient add / f");
  LpipsConvParams p{x, wp, bias, add, f, out, NI * H * W, H, W, Cin, Cout};
  ONIRIS_CHECK_ARG((p.M + LPIPS_TM_SMALL - 1) / LPIPS_TM_SMALL <= 0x7fffffffLL, "lpips_conv: %lld pixels", p.M);
  // 256-row tiles unless they would leave CUs idle (fewer workgroups than the 256 CUs): the same bits either way
  if (tile == 0) tile = (p.M + LPIPS_TM - 1) / LPIPS_TM * (Cout / LPIPS_WN) < 256 ? LPIPS_TM_SMALL : LPIPS_TM;
  if (ksize == 5 && mode == LPIPS_EPI_FWD) lpips_conv_launch<5, LPIPS_EPI_FWD>(p, tile, (hipStream_t)stream);
  else if (ksize == 5) lpips_conv_launch<5, LPIPS_EPI_BWD>(p, tile, (hipStream_t)stream);
  else if (mode == LPIPS_EPI_FWD) lpips_conv_launch<3, LPIPS_EPI_FWD>(p, tile, (hipStream_t)stream);
  else lpips_conv_launch<3, LPIPS_EPI_BWD>(p, tile, (hipStream_t)stream);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_lpips_pool(const float* x, float* out, int NI, int H, int W, int C, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && out && NI > 0 && H >= 3 && W >= 3 && C > 0 && C % 4 == 0, "lpips_pool: bad arguments");
  const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
  const long long total = (long long)NI * Ho * Wo * (C / 4);
  ONIRIS_CHECK_ARG((total + 255) / 256 <= 0x7fffffffLL, "lpips_pool: %lld elements", total);
  ONIRIS_KLAUNCH(lpips_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, H, W, Ho, Wo, C / 4,
                 total);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_lpips_pool_bwd(const float* dp, const float* f, const float* add, int mask, float* out, int NI, int H, int W,
                                     int C, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(dp && f && out && NI > 0 && H >= 3 && W >= 3 && C > 0 && C % 4 == 0, "lpips_pool_bwd: bad arguments");
  const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
  const long long total = (long long)NI * H * W * (C / 4);
  ONIRIS_CHECK_ARG((total + 255) / 256 <= 0x7fffffffLL, "lpips_pool_bwd: %lld elements", total);
  ONIRIS_KLAUNCH(lpips_pool_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dp, f, add, mask, out,
                 H, W, Ho, Wo, C / 4, total);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

static inline bool lpips_head_c_ok(int C) { return C > 0 && C % 64 == 0 && C <= 64 * HEAD_CPL; }

extern "C" int oniris_lpips_head_fwd(const float* fa, const float* fb, const float* w, float* part, int N, int HW, int C,
                                     oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(fa && fb && w && part && N > 0 && HW > 0, "lpips_head_fwd: bad arguments");
  ONIRIS_CHECK_ARG(lpips_head_c_ok(C) && N <= 65535, "lpips_head_fwd: C %d (a multiple of 64 up to 384), N %d (up to 65535)", C, N);
  const int P = cdiv(HW, HEAD_PIX);
  ONIRIS_KLAUNCH(lpips_head_fwd_kernel, dim3(P, N), dim3(256), 0, (hipStream_t)stream, fa, fb, w, part, HW, C, P);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_lpips_head_sum(const float* part, int layers, const long long* off, const int* HW, int N, float* out,
                                     oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(part && off && HW && out && N > 0 && layers > 0 && layers <= 8, "lpips_head_sum: bad arguments");
  LpipsHeadSumParams p;
  p.layers = layers;
  for (int k = 0; k < layers; ++k) {
    ONIRIS_CHECK_ARG(HW[k] > 0 && off[k] >= 0, "lpips_head_sum: layer %d", k);
    p.off[k] = off[k];
    p.HW[k] = HW[k];
    p.P[k] = cdiv(HW[k], HEAD_PIX);
  }
  ONIRIS_KLAUNCH(lpips_head_sum_kernel, dim3(cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, part, p, N, out);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_lpips_head_bwd(const float* fa, const float* fb, const float* w, const float* cot, float* ga, float* gb, int mask,
                                     int N, int HW, int C, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(fa && fb && w && cot && (ga || gb) && N > 0 && HW > 0, "lpips_head_bwd: bad arguments");
  ONIRIS_CHECK_ARG(lpips_head_c_ok(C) && N <= 65535, "lpips_head_bwd: C %d (a multiple of 64 up to 384), N %d (up to 65535)", C, N);
  ONIRIS_KLAUNCH(lpips_head_bwd_kernel, dim3(cdiv(HW, HEAD_PIX), N), dim3(256), 0, (hipStream_t)stream, fa, fb, w, cot, ga, gb, mask, HW,
                 C);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}
