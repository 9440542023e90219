// VAE discriminator, the spatio-temporal half (reference: edm2/vae/discriminator.py Discriminator3D :242-283, DiscriminatorBlock3D
// :181-239, BlurPooling3D), fp32 throughout, channels-last activations [N][T][H][W][C].  include/oniris.h: oniris_disc3d_*.
//   oniris_disc3d_conv             27-tap conv, stride 1 (forward and data gradient) or 2 (the stem), on the f32 MFMA with the
//                                  per-sample GroupNorm + LeakyReLU prologue, bias / residual epilogue and per-tile statistics
//                                  (csrc/disc_conv3d.h over csrc/disc_parts.h)
//   oniris_disc3d_wgrad            its weight and bias gradient into a bounded number of slabs
//   oniris_disc3d_stem_dgrad       the stem's data gradient (at most 8 channels out): plain FMA, gathered per input element
//   oniris_disc3d_gn_finalize      tile partials -> per (sample, group) mean / var / rstd and the prologue vectors s, t
//   oniris_disc3d_gn_bwd_reduce / _gn_bwd_finalize / _gn_bwd_dx    GroupNorm + LeakyReLU backward
//   oniris_disc3d_blur / _blur_bwd [1,2,1]^3 / 64, stride 2, pad 1, with the prologue; its transpose in gather form
// The 1x1x1 shortcut convs are oniris_disc_conv / oniris_disc_wgrad over the N T planes.  Every sum has a fixed order and no atomic
// is used: two runs give the same bits.
#include "oniris.h"
#include "common.h"
#include "disc_conv3d.h"

#define DISC3D_GROUPS 32

template <int NB, int S>
static int disc3d_conv_launch(const Disc3dConvParams& p, dim3 grid, hipStream_t stream) {
  constexpr int HS = 15 * S + 3, AP = S == 1 ? DISC_APITCH : 9, WP = NB == 2 ? 96 : 32;
  const size_t bytes = ((size_t)HS * HS * AP + (size_t)9 * DISC_KC * WP) * sizeof(float);
  if (int rc = disc_raise_lds(disc3d_conv_kernel<NB, S>, bytes, "disc3d_conv")) return rc;
  ONIRIS_KLAUNCH((disc3d_conv_kernel<NB, S>), grid, dim3(256), bytes, stream, p);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_disc3d_conv(const float* x, const float* w, const float* bias, const float* pro_s, const float* pro_t,
                                  const float* res, float res_scale, float* out, float* part, int N, int T, int H, int W, int Cin,
                                  int Cout, int stride, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && w && out && N > 0 && T > 0 && H > 0 && W > 0 && (stride == 1 || stride == 2), "disc3d_conv: bad arguments");
  ONIRIS_CHECK_ARG(disc_c_ok(Cin) && disc_c_ok(Cout), "disc3d_conv: Cin %d / Cout %d: 1..8 or a multiple of 32", Cin, Cout);
  ONIRIS_CHECK_ARG(stride == 1 || (Cin <= 8 && Cout % 32 == 0 && !pro_s && !res),
                   "disc3d_conv: stride 2 takes Cin 1..8, Cout %% 32 == 0, no prologue and no residual");
  ONIRIS_CHECK_ARG(!pro_s == !pro_t, "disc3d_conv: the prologue needs both s and t");
  ONIRIS_CHECK_ARG(!part || Cout % 32 == 0, "disc3d_conv: statistics need Cout %% 32 == 0");
  Disc3dConvParams p;
  p.x = x; p.w = w; p.bias = bias; p.pro_s = pro_s; p.pro_t = pro_t; p.res = res; p.out = out; p.part = part;
  p.N = N; p.T = T; p.H = H; p.W = W; p.To = disc_out(T, stride); p.Ho = disc_out(H, stride); p.Wo = disc_out(W, stride);
  p.Cin = Cin; p.CinP = Cin <= 8 ? 8 : Cin; p.Cout = Cout; p.CoutP = roundup(Cout, 32);
  p.tiles_x = cdiv(p.Wo, DISC_TILE); p.tiles_y = cdiv(p.Ho, DISC_TILE); p.res_scale = res_scale;
  const long long wgs = (long long)N * p.To * p.tiles_x * p.tiles_y;
  ONIRIS_CHECK_ARG(wgs <= 0x7fffffffLL && (long long)N * T <= 0x7fffffffLL, "disc3d_conv: %lld tiles", wgs);
  const int nb = p.CoutP % 64 == 0 ? 2 : 1;
  const dim3 grid((unsigned)wgs, p.CoutP / (32 * nb));
  if (stride == 1) return nb == 2 ? disc3d_conv_launch<2, 1>(p, grid, (hipStream_t)stream) : disc3d_conv_launch<1, 1>(p, grid, (hipStream_t)stream);
  return nb == 2 ? disc3d_conv_launch<2, 2>(p, grid, (hipStream_t)stream) : disc3d_conv_launch<1, 2>(p, grid, (hipStream_t)stream);
}

template <int S>
static int disc3d_wgrad_launch(const Disc3dWgradParams& p, dim3 grid, hipStream_t stream) {
  constexpr int HS = 15 * S + 3, AP = S == 1 ? DISC_WPITCH : 9;
  const size_t bytes = ((size_t)HS * HS * AP + 256 * 32) * sizeof(float);
  if (int rc = disc_raise_lds(disc3d_wgrad_kernel<S>, bytes, "disc3d_wgrad")) return rc;
  ONIRIS_KLAUNCH((disc3d_wgrad_kernel<S>), grid, dim3(256), bytes, stream, p);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_disc3d_wgrad(const float* x, const float* pro_s, const float* pro_t, const float* dy, float* slab, int nslab,
                                   int N, int T, int H, int W, int Cin, int Cout, int stride, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && dy && slab && nslab > 0 && N > 0 && T > 0 && H > 0 && W > 0 && (stride == 1 || stride == 2),
                   "disc3d_wgrad: bad arguments");
  ONIRIS_CHECK_ARG(disc_c_ok(Cin) && disc_c_ok(Cout), "disc3d_wgrad: Cin %d / Cout %d: 1..8 or a multiple of 32", Cin, Cout);
  ONIRIS_CHECK_ARG(stride == 1 || (Cin <= 8 && !pro_s), "disc3d_wgrad: stride 2 takes Cin 1..8 and no prologue");
  ONIRIS_CHECK_ARG(!pro_s == !pro_t, "disc3d_wgrad: the prologue needs both s and t");
  Disc3dWgradParams p;
  p.x = x; p.pro_s = pro_s; p.pro_t = pro_t; p.dy = dy; p.slab = slab;
  p.N = N; p.T = T; p.H = H; p.W = W; p.To = disc_out(T, stride); p.Ho = disc_out(H, stride); p.Wo = disc_out(W, stride);
  p.Cin = Cin; p.CinP = Cin <= 8 ? 8 : Cin; p.Cout = Cout;
  p.tiles_x = cdiv(p.Wo, DISC_TILE); p.tiles_y = cdiv(p.Ho, DISC_TILE);
  const long long items = (long long)N * p.To * p.tiles_x * p.tiles_y;
  ONIRIS_CHECK_ARG(items <= 0x7fffffffLL && (long long)N * T <= 0x7fffffffLL, "disc3d_wgrad: %lld work items", items);
  p.nitems = (int)items; p.nslab = nslab; p.ncib = cdiv(p.CinP, DISC_WKC);
  p.slab_size = 27LL * Cin * Cout + Cout;
  const dim3 grid(nslab, 3 * p.ncib, cdiv(Cout, 32));
  return stride == 1 ? disc3d_wgrad_launch<1>(p, grid, (hipStream_t)stream) : disc3d_wgrad_launch<2>(p, grid, (hipStream_t)stream);
}

// ---- the stem's data gradient: dx[n][t][y][x][ci] = sum over the (output position, tap) pairs that read this input element, kt
// then ky then kx ascending, and within a pair over co ascending, of dy[..][co] w[tap][ci][co] (w in the forward layout)
__global__ __launch_bounds__(256) void disc3d_stem_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                                float* __restrict__ dx, int T, int H, int W, int To, int Ho, int Wo,
                                                                int Cin, int Cout, long long total) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int ci = (int)(e % Cin);
  long long r = e / Cin;
  const int xx = (int)(r % W); r /= W;
  const int y = (int)(r % H); r /= H;
  const int t = (int)(r % T);
  const long long n = r / T;
  float acc = 0.f;
  for (int kt = 0; kt < 3; ++kt) {
    const int tt = t + 1 - kt;
    if (tt < 0 || (tt & 1) || (tt >> 1) >= To) continue;
    for (int ky = 0; ky < 3; ++ky) {
      const int yy = y + 1 - ky;
      if (yy < 0 || (yy & 1) || (yy >> 1) >= Ho) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int xo = xx + 1 - kx;
        if (xo < 0 || (xo & 1) || (xo >> 1) >= Wo) continue;
        const float* d = dy + (((n * To + (tt >> 1)) * Ho + (yy >> 1)) * Wo + (xo >> 1)) * Cout;
        const float* wv = w + ((size_t)((kt * 3 + ky) * 3 + kx) * 8 + ci) * Cout;
        for (int co = 0; co < Cout; co += 4) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(d + co), b = *reinterpret_cast<const f32x4*>(wv + co);
#pragma unroll
          for (int k = 0; k < 4; ++k) acc = __builtin_fmaf(a[k], b[k], acc);
        }
      }
    }
  }
  dx[e] = acc;
}

extern "C" int oniris_disc3d_stem_dgrad(const float* dy, const float* w, float* dx, int N, int T, int H, int W, int Cin, int Cout,
                                        oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(dy && w && dx && N > 0 && T > 0 && H > 0 && W > 0 && Cin >= 1 && Cin <= 8 && Cout > 0 && Cout % 32 == 0,
                   "disc3d_stem_dgrad: bad arguments (Cin 1..8, Cout %% 32 == 0)");
  const long long total = (long long)N * T * H * W * Cin;
  ONIRIS_CHECK_ARG((total + 255) / 256 <= 0x7fffffffLL, "disc3d_stem_dgrad: %lld elements", total);
  ONIRIS_KLAUNCH(disc3d_stem_dgrad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, w, dx, T, H,
                 W, disc_out(T, 2), disc_out(H, 2), disc_out(W, 2), Cin, Cout, total);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

// ---- GroupNorm statistics: disc_chan over the P tile partials of one sample times the C / 32 channels of one group; thread t takes
// entries t, t + 256, ... (entry = partial * cpg + channel) in order, then a fixed tree

__global__ __launch_bounds__(256) void disc3d_gn_finalize_kernel(const float* __restrict__ part, int N, int P, int C,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 float eps, float* __restrict__ stats) {
  __shared__ double sn[256], sm[256], sq[256];
  const int g = blockIdx.x, smp = blockIdx.y, t = threadIdx.x, cpg = C / DISC3D_GROUPS;
  double n = 0.0, m = 0.0, q = 0.0;
  for (int i = t; i < P * cpg; i += 256) {
    const float* e = part + ((size_t)smp * P + i / cpg) * 4 * C + g * cpg + i % cpg;
    const double cnt = e[0], s1 = e[3 * C];
    disc_chan(n, m, q, cnt, (double)e[C] + s1 / cnt, (double)e[2 * C] - s1 * s1 / cnt);
  }
  sn[t] = n; sm[t] = m; sq[t] = q;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      disc_chan(n, m, q, sn[t + s], sm[t + s], sq[t + s]);
      sn[t] = n; sm[t] = m; sq[t] = q;
    }
    __syncthreads();
  }
  if (t < cpg) {
    const int c = g * cpg + t;
    const size_t NC = (size_t)N * C, o = (size_t)smp * C + c;
    const double mean = sm[0], var = sq[0] / sn[0];
    const double rstd = 1.0 / sqrt(var + (double)eps);
    const double s = (double)gamma[c] * rstd;
    stats[o] = (float)mean;
    stats[NC + o] = (float)var;
    stats[2 * NC + o] = (float)s;
    stats[3 * NC + o] = (float)((double)beta[c] - mean * s);
    stats[4 * NC + o] = (float)rstd;
  }
}

extern "C" int oniris_disc3d_gn_finalize(const float* part, int N, int P, int C, const float* gamma, const float* beta, float eps,
                                         float* stats, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(part && gamma && beta && stats && N > 0 && P > 0 && C > 0 && C % DISC3D_GROUPS == 0 && C <= 256 && N <= 65535,
                   "disc3d_gn_finalize: bad arguments (C a multiple of 32 up to 256)");
  ONIRIS_KLAUNCH(disc3d_gn_finalize_kernel, dim3(DISC3D_GROUPS, N), dim3(256), 0, (hipStream_t)stream, part, N, P, C, gamma, beta, eps,
                 stats);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

// ---- GroupNorm + LeakyReLU backward.  stats = [mean | var | s | t | rstd][N][C] as oniris_disc3d_gn_finalize writes them.
// per (sample, group): the channel sums S1 = sum dz, S2 = sum dz xhat (thread t takes partials t, t + 256, ..., then a fixed tree),
// and the group means m1 = sum_c gamma S1 / cnt, m2 = sum_c gamma S2 / cnt, channels ascending
__global__ __launch_bounds__(256) void disc3d_gn_bwd_finalize_kernel(const float* __restrict__ part, int N, int P, int C,
                                                                     const float* __restrict__ gamma, float inv_cnt,
                                                                     float* __restrict__ sums, float* __restrict__ mm) {
  __shared__ float r1[256], r2[256];
  const int g = blockIdx.x, smp = blockIdx.y, t = threadIdx.x, cpg = C / DISC3D_GROUPS;
  float m1 = 0.f, m2 = 0.f;
  for (int cc = 0; cc < cpg; ++cc) {
    const int c = g * cpg + cc;
    float a = 0.f, b = 0.f;
    for (int i = t; i < P; i += 256) {
      const float* e = part + ((size_t)smp * P + i) * 2 * C;
      a += e[c];
      b += e[C + c];
    }
    __syncthreads();
    r1[t] = a; r2[t] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (t < s) { r1[t] += r1[t + s]; r2[t] += r2[t + s]; }
      __syncthreads();
    }
    if (t == 0) {
      sums[(size_t)smp * 2 * C + c] = r1[0];
      sums[(size_t)smp * 2 * C + C + c] = r2[0];
      m1 = __builtin_fmaf(gamma[c], r1[0], m1);
      m2 = __builtin_fmaf(gamma[c], r2[0], m2);
    }
  }
  if (t == 0) {
    mm[(size_t)smp * DISC3D_GROUPS + g] = m1 * inv_cnt;
    mm[((size_t)N + smp) * DISC3D_GROUPS + g] = m2 * inv_cnt;
  }
}

__global__ __launch_bounds__(256) void disc3d_gn_bwd_dx_kernel(const float* __restrict__ da, const float* __restrict__ z,
                                                               const float* __restrict__ stats, const float* __restrict__ gamma,
                                                               const float* __restrict__ mm, const float* __restrict__ add,
                                                               float add_scale, float* __restrict__ dx, int N, long long per_sample,
                                                               long long total, int C) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C), smp = (int)(e / per_sample), g = c / (C / DISC3D_GROUPS);
  const size_t NC = (size_t)N * C, o = (size_t)smp * C + c;
  const float mean = stats[o], s = stats[2 * NC + o], t = stats[3 * NC + o], rstd = stats[4 * NC + o];
  const float m1 = mm[(size_t)smp * DISC3D_GROUPS + g], m2 = mm[((size_t)N + smp) * DISC3D_GROUPS + g];
  const float zv = z[e], gv = da[e];
  const float dz = disc_dz(zv, s, t, gv);
  const float xh = (zv - mean) * rstd;
  float v = rstd * ((gamma[c] * dz - m1) - xh * m2);
  if (add) v = __builtin_fmaf(add_scale, add[e], v);
  dx[e] = v;
}

extern "C" int oniris_disc3d_gn_bwd_reduce(const float* da, const float* z, const float* stats, float* part, int N, int64_t npix,
                                           int C, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(da && z && stats && part && N > 0 && N <= 65535 && npix > 0 && C > 0, "disc3d_gn_bwd_reduce: bad arguments");
  return disc3d_gn_bwd_reduce_launch("disc3d_gn_bwd_reduce", da, z, stats, part, N, (long long)npix, C, (hipStream_t)stream);
}

extern "C" int oniris_disc3d_gn_bwd_finalize(const float* part, int N, int P, int C, const float* gamma, int64_t npix, float* sums,
                                             float* mm, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(part && gamma && sums && mm && N > 0 && N <= 65535 && P > 0 && npix > 0 && C > 0 && C % DISC3D_GROUPS == 0,
                   "disc3d_gn_bwd_finalize: bad arguments (C a multiple of 32)");
  const float inv_cnt = (float)(1.0 / ((double)npix * (C / DISC3D_GROUPS)));
  ONIRIS_KLAUNCH(disc3d_gn_bwd_finalize_kernel, dim3(DISC3D_GROUPS, N), dim3(256), 0, (hipStream_t)stream, part, N, P, C, gamma,
                 inv_cnt, sums, mm);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_disc3d_gn_bwd_dx(const float* da, const float* z, const float* stats, const float* gamma, const float* mm,
                                       const float* add, float add_scale, float* dx, int N, int64_t npix, int C,
                                       oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(da && z && stats && gamma && mm && dx && N > 0 && npix > 0 && C > 0 && C % DISC3D_GROUPS == 0,
                   "disc3d_gn_bwd_dx: bad arguments (C a multiple of 32)");
  const long long per_sample = (long long)npix * C, total = per_sample * N;
  ONIRIS_CHECK_ARG((total + 255) / 256 <= 0x7fffffffLL, "disc3d_gn_bwd_dx: %lld elements", total);
  ONIRIS_KLAUNCH(disc3d_gn_bwd_dx_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, da, z, stats,
                 gamma, mm, add, add_scale, dx, N, per_sample, total, C);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

// ---- 3-D blur pool and its transpose; the filter weight of tap (i, j, k) is wt(i) wt(j) wt(k) / 64, wt = 1, 2, 1
__global__ __launch_bounds__(256) void disc3d_blur_kernel(const float* __restrict__ x, const float* __restrict__ pro_s,
                                                          const float* __restrict__ pro_t, float* __restrict__ out, int T, int H,
                                                          int W, int C, int To, int Ho, int Wo, long long total) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  long long r = e / C;
  const int ox = (int)(r % Wo); r /= Wo;
  const int oy = (int)(r % Ho); r /= Ho;
  const int ot = (int)(r % To);
  const long long n = r / To;
  float s = 1.f, t = 0.f;
  if (pro_s) { s = pro_s[n * C + c]; t = pro_t[n * C + c]; }
  float acc = 0.f;
  for (int l = 0; l < 3; ++l) {
    const int tt = 2 * ot - 1 + l;
    if (tt < 0 || tt >= T) continue;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int y = 2 * oy - 1 + i;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int xx = 2 * ox - 1 + k;
        if (y < 0 || y >= H || xx < 0 || xx >= W) continue;
        float v = x[(((n * T + tt) * H + y) * W + xx) * C + c];
        if (pro_s) v = disc_act(v, s, t);
        acc = __builtin_fmaf((float)((l == 1 ? 2 : 1) * (i == 1 ? 2 : 1) * (k == 1 ? 2 : 1)) * 0.015625f, v, acc);
      }
    }
  }
  out[e] = acc;
}

__global__ __launch_bounds__(256) void disc3d_blur_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int T, int H, int W,
                                                              int C, int To, int Ho, int Wo, long long total) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  long long r = e / C;
  const int xx = (int)(r % W); r /= W;
  const int y = (int)(r % H); r /= H;
  const int t = (int)(r % T);
  const long long n = r / T;
  float acc = 0.f;
  for (int ot = t >> 1; ot <= (t + 1) >> 1; ++ot) {
    if (ot >= To) continue;
    const int l = t + 1 - 2 * ot;
    for (int oy = y >> 1; oy <= (y + 1) >> 1; ++oy) {
      if (oy >= Ho) continue;
      const int i = y + 1 - 2 * oy;
      for (int ox = xx >> 1; ox <= (xx + 1) >> 1; ++ox) {
        if (ox >= Wo) continue;
        const int k = xx + 1 - 2 * ox;
        acc = __builtin_fmaf((float)((l == 1 ? 2 : 1) * (i == 1 ? 2 : 1) * (k == 1 ? 2 : 1)) * 0.015625f,
                             dy[(((n * To + ot) * Ho + oy) * Wo + ox) * C + c], acc);
      }
    }
  }
  dx[e] = acc;
}

extern "C" int oniris_disc3d_blur(const float* x, const float* pro_s, const float* pro_t, float* out, int N, int T, int H, int W,
                                  int C, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && out && N > 0 && T > 0 && H > 0 && W > 0 && C > 0 && !pro_s == !pro_t, "disc3d_blur: bad arguments");
  const int To = disc_out(T, 2), Ho = disc_out(H, 2), Wo = disc_out(W, 2);
  const long long total = (long long)N * To * Ho * Wo * C;
  ONIRIS_CHECK_ARG((total + 255) / 256 <= 0x7fffffffLL, "disc3d_blur: %lld elements", total);
  ONIRIS_KLAUNCH(disc3d_blur_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, pro_s, pro_t, out, T,
                 H, W, C, To, Ho, Wo, total);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_disc3d_blur_bwd(const float* dy, float* dx, int N, int T, int H, int W, int C, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(dy && dx && N > 0 && T > 0 && H > 0 && W > 0 && C > 0, "disc3d_blur_bwd: bad arguments");
  const int To = disc_out(T, 2), Ho = disc_out(H, 2), Wo = disc_out(W, 2);
  const long long total = (long long)N * T * H * W * C;
  ONIRIS_CHECK_ARG((total + 255) / 256 <= 0x7fffffffLL, "disc3d_blur_bwd: %lld elements", total);
  ONIRIS_KLAUNCH(disc3d_blur_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, dx, T, H, W, C,
                 To, Ho, Wo, total);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}
