// VAE discriminator, the per-frame half (reference: edm2/vae/discriminator.py Discriminator2D :70-111, DiscriminatorBlock2D
// :11-67, BlurPooling2D :154-178), fp32 throughout, channels-last activations [N][H][W][C].  include/oniris.h: oniris_disc_*.
//   oniris_disc_conv            3x3 / 1x1 conv on the f32 MFMA with the BatchNorm + LeakyReLU prologue, bias / residual epilogue and
//                               per-workgroup (count, centre, S2, S1) of what it stores (csrc/disc_conv3.h over csrc/disc_parts.h);
//                               the data gradient is the same launch on flipped, transposed weights
//   oniris_disc_stats_finalize  partials -> mean, biased var, s = gamma rstd, t = beta - mean s, rstd; running buffers
//   oniris_disc_blur / _bwd     [1,2,1] x [1,2,1] / 16, stride 2, pad 1, with the same prologue; its transpose in gather form
//   oniris_disc_bn_bwd_reduce   per-workgroup sums of dz and dz xhat, dz = da lrelu'(z s + t): the GroupNorm reduce at one sample
//   oniris_disc_part_sum        the sum of such partials, in a fixed tree order
//   oniris_disc_bn_bwd_dx       dx = s (dz - mean(dz) - xhat mean(dz xhat)) (+ add_scale add)
//   oniris_disc_wgrad           weight and bias gradient into a bounded number of slabs (summed by oniris_vae_slab_sum_bwd)
// Every sum has a fixed order and no atomic is used: two runs give the same bits.
#include "oniris.h"
#include "common.h"
#include "disc_conv3.h"

template <int NB>
static int disc_conv_launch(const DiscConvParams& p, dim3 grid, hipStream_t stream) {
  constexpr int WP = NB == 2 ? 96 : 32;
  const size_t bytes = ((size_t)DISC_HALO * DISC_HALO * DISC_APITCH + (size_t)p.taps * DISC_KC * WP) * sizeof(float);
  if (int rc = disc_raise_lds(disc_conv_kernel<NB>, bytes, "disc_conv")) return rc;
  ONIRIS_KLAUNCH(disc_conv_kernel<NB>, grid, dim3(256), bytes, stream, p);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_disc_conv(const float* x, const float* w, const float* bias, const float* pro_s, const float* pro_t,
                                const float* res, float res_scale, float* out, float* part, int N, int H, int W, int Cin, int Cout,
                                int taps, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && w && out && N > 0 && H > 0 && W > 0 && (taps == 1 || taps == 9), "disc_conv: bad arguments");
  ONIRIS_CHECK_ARG(disc_c_ok(Cin) && disc_c_ok(Cout), "disc_conv: Cin %d / Cout %d: 1..8 or a multiple of 32", Cin, Cout);
  ONIRIS_CHECK_ARG(!pro_s == !pro_t, "disc_conv: the prologue needs both s and t");
  ONIRIS_CHECK_ARG(!part || Cout % 32 == 0, "disc_conv: statistics need Cout %% 32 == 0");
  DiscConvParams p;
  p.x = x; p.w = w; p.bias = bias; p.pro_s = pro_s; p.pro_t = pro_t; p.res = res; p.out = out; p.part = part;
  p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.CinP = Cin <= 8 ? 8 : Cin; p.Cout = Cout; p.CoutP = roundup(Cout, 32); p.taps = taps;
  p.tiles_x = cdiv(W, DISC_TILE); p.tiles_y = cdiv(H, DISC_TILE); p.res_scale = res_scale;
  const long long wgs = (long long)N * p.tiles_x * p.tiles_y;
  ONIRIS_CHECK_ARG(wgs <= 0x7fffffffLL, "disc_conv: %lld tiles", wgs);
  const int nb = p.CoutP % 64 == 0 ? 2 : 1;
  const dim3 grid((unsigned)wgs, p.CoutP / (32 * nb));
  return nb == 2 ? disc_conv_launch<2>(p, grid, (hipStream_t)stream) : disc_conv_launch<1>(p, grid, (hipStream_t)stream);
}

template <int TAPS>
static int disc_wgrad_launch(const DiscWgradParams& p, dim3 grid, hipStream_t stream) {
  const size_t bytes = ((size_t)DISC_HALO * DISC_HALO * DISC_WPITCH + 256 * 32) * sizeof(float);
  if (int rc = disc_raise_lds(disc_wgrad_kernel<TAPS>, bytes, "disc_wgrad")) return rc;
  ONIRIS_KLAUNCH(disc_wgrad_kernel<TAPS>, grid, dim3(256), bytes, stream, p);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_disc_wgrad(const float* x, const float* pro_s, const float* pro_t, const float* dy, float* slab, int nslab,
                                 int N, int H, int W, int Cin, int Cout, int taps, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && dy && slab && nslab > 0 && N > 0 && H > 0 && W > 0 && (taps == 1 || taps == 9), "disc_wgrad: bad arguments");
  ONIRIS_CHECK_ARG(disc_c_ok(Cin) && disc_c_ok(Cout), "disc_wgrad: Cin %d / Cout %d: 1..8 or a multiple of 32", Cin, Cout);
  ONIRIS_CHECK_ARG(!pro_s == !pro_t, "disc_wgrad: the prologue needs both s and t");
  DiscWgradParams p;
  p.x = x; p.pro_s = pro_s; p.pro_t = pro_t; p.dy = dy; p.slab = slab;
  p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.CinP = Cin <= 8 ? 8 : Cin; p.Cout = Cout;
  p.tiles_x = cdiv(W, DISC_TILE); p.tiles_y = cdiv(H, DISC_TILE);
  const long long items = (long long)N * p.tiles_x * p.tiles_y;
  ONIRIS_CHECK_ARG(items <= 0x7fffffffLL, "disc_wgrad: %lld work items", items);
  p.nitems = (int)items; p.nslab = nslab;
  p.slab_size = (long long)taps * Cin * Cout + Cout;
  const dim3 grid(nslab, cdiv(p.CinP, DISC_WKC), cdiv(Cout, 32));
  return taps == 9 ? disc_wgrad_launch<9>(p, grid, (hipStream_t)stream) : disc_wgrad_launch<1>(p, grid, (hipStream_t)stream);
}

// ---- statistics: disc_chan over the partials of one channel, thread t takes partials t, t + 256, ... in order, then a fixed tree

__global__ __launch_bounds__(256) void disc_stats_finalize_kernel(const float* __restrict__ part, int P, int C,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  float* running_mean, float* running_var, float momentum, float eps,
                                                                  float* __restrict__ stats) {
  __shared__ double sn[256], sm[256], sq[256];
  const int c = blockIdx.x, t = threadIdx.x;
  double n = 0.0, m = 0.0, q = 0.0;
  for (int i = t; i < P; i += 256) {
    const float* e = part + (size_t)i * 4 * C + c;
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
  if (t == 0) {
    const double var = q / n;
    const double rstd = 1.0 / sqrt(var + (double)eps);
    const double s = (double)gamma[c] * rstd;
    stats[c] = (float)m;
    stats[C + c] = (float)var;
    stats[2 * C + c] = (float)s;
    stats[3 * C + c] = (float)((double)beta[c] - m * s);
    stats[4 * C + c] = (float)rstd;
    if (running_mean) {
      running_mean[c] = (float)((1.0 - (double)momentum) * running_mean[c] + (double)momentum * m);
      running_var[c] = (float)((1.0 - (double)momentum) * running_var[c] + (double)momentum * (q / (n - 1.0)));
    }
  }
}

extern "C" int oniris_disc_stats_finalize(const float* part, int P, int C, const float* gamma, const float* beta,
                                          float* running_mean, float* running_var, float momentum, float eps, float* stats,
                                          oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(part && gamma && beta && stats && P > 0 && C > 0 && !running_mean == !running_var,
                   "disc_stats_finalize: bad arguments");
  ONIRIS_KLAUNCH(disc_stats_finalize_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, part, P, C, gamma, beta, running_mean,
                 running_var, momentum, eps, stats);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

// ---- out[e] = sum_p part[p][e]: thread t takes p = t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void disc_part_sum_kernel(const float* __restrict__ part, int P, int n, float* __restrict__ out) {
  __shared__ float sv[256];
  const int e = blockIdx.x, t = threadIdx.x;
  float v = 0.f;
  for (int i = t; i < P; i += 256) v += part[(size_t)i * n + e];
  sv[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sv[t] = sv[t] + sv[t + s];
    __syncthreads();
  }
  if (t == 0) out[e] = sv[0];
}

extern "C" int oniris_disc_part_sum(const float* part, int P, int n, float* out, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(part && out && P > 0 && n > 0, "disc_part_sum: bad arguments");
  ONIRIS_KLAUNCH(disc_part_sum_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, part, P, n, out);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

// ---- blur pool and its transpose
__global__ __launch_bounds__(256) void disc_blur_kernel(const float* __restrict__ x, const float* __restrict__ pro_s,
                                                        const float* __restrict__ pro_t, float* __restrict__ out, int H, int W, int C,
                                                        int Ho, int Wo, long long total) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  long long r = e / C;
  const int ox = (int)(r % Wo); r /= Wo;
  const int oy = (int)(r % Ho);
  const long long n = r / Ho;
  float s = 1.f, t = 0.f;
  if (pro_s) { s = pro_s[c]; t = pro_t[c]; }
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int y = 2 * oy - 1 + i;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int xx = 2 * ox - 1 + k;
      if (y < 0 || y >= H || xx < 0 || xx >= W) continue;
      float v = x[((n * H + y) * W + xx) * C + c];
      if (pro_s) v = disc_act(v, s, t);
      acc = __builtin_fmaf((float)((i == 1 ? 2 : 1) * (k == 1 ? 2 : 1)) * 0.0625f, v, acc);
    }
  }
  out[e] = acc;
}

__global__ __launch_bounds__(256) void disc_blur_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int H, int W, int C,
                                                            int Ho, int Wo, long long total) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  long long r = e / C;
  const int xx = (int)(r % W); r /= W;
  const int y = (int)(r % H);
  const long long n = r / H;
  float acc = 0.f;
  for (int oy = y >> 1; oy <= (y + 1) >> 1; ++oy) {
    if (oy >= Ho) continue;
    const int i = y + 1 - 2 * oy;
    for (int ox = xx >> 1; ox <= (xx + 1) >> 1; ++ox) {
      if (ox >= Wo) continue;
      const int k = xx + 1 - 2 * ox;
      acc = __builtin_fmaf((float)((i == 1 ? 2 : 1) * (k == 1 ? 2 : 1)) * 0.0625f, dy[((n * Ho + oy) * Wo + ox) * C + c], acc);
    }
  }
  dx[e] = acc;
}

extern "C" int oniris_disc_blur(const float* x, const float* pro_s, const float* pro_t, float* out, int N, int H, int W, int C,
                                oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && out && N > 0 && H > 0 && W > 0 && C > 0 && !pro_s == !pro_t, "disc_blur: bad arguments");
  const int Ho = disc_out(H, 2), Wo = disc_out(W, 2);
  const long long total = (long long)N * Ho * Wo * C;
  ONIRIS_CHECK_ARG((total + 255) / 256 <= 0x7fffffffLL, "disc_blur: %lld elements", total);
  ONIRIS_KLAUNCH(disc_blur_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, pro_s, pro_t, out, H,
                 W, C, Ho, Wo, total);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_disc_blur_bwd(const float* dy, float* dx, int N, int H, int W, int C, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(dy && dx && N > 0 && H > 0 && W > 0 && C > 0, "disc_blur_bwd: bad arguments");
  const int Ho = disc_out(H, 2), Wo = disc_out(W, 2);
  const long long total = (long long)N * H * W * C;
  ONIRIS_CHECK_ARG((total + 255) / 256 <= 0x7fffffffLL, "disc_blur_bwd: %lld elements", total);
  ONIRIS_KLAUNCH(disc_blur_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, dx, H, W, C, Ho,
                 Wo, total);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

// ---- BatchNorm + LeakyReLU backward.  stats = [mean | var | s | t | rstd][C] as oniris_disc_stats_finalize writes them.
__global__ __launch_bounds__(256) void disc_bn_bwd_dx_kernel(const float* __restrict__ da, const float* __restrict__ z,
                                                             const float* __restrict__ stats, const float* __restrict__ sums,
                                                             const float* __restrict__ add, float add_scale, float* __restrict__ dx,
                                                             long long total, int C, float inv_n, int eval) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  const float mean = stats[c], s = stats[2 * C + c], t = stats[3 * C + c], rstd = stats[4 * C + c];
  const float zv = z[e], g = da[e];
  const float dz = disc_dz(zv, s, t, g);
  float v;
  if (eval) {
    v = s * dz;
  } else {
    const float xh = (zv - mean) * rstd;
    v = s * ((dz - sums[c] * inv_n) - xh * (sums[C + c] * inv_n));
  }
  if (add) v = __builtin_fmaf(add_scale, add[e], v);
  dx[e] = v;
}

extern "C" int oniris_disc_bn_bwd_reduce(const float* da, const float* z, const float* stats, float* part, int64_t npix, int C,
                                         oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(da && z && stats && part && npix > 0 && C > 0, "disc_bn_bwd_reduce: bad arguments");
  return disc3d_gn_bwd_reduce_launch("disc_bn_bwd_reduce", da, z, stats, part, 1, (long long)npix, C, (hipStream_t)stream);
}

extern "C" int oniris_disc_bn_bwd_dx(const float* da, const float* z, const float* stats, const float* sums, const float* add,
                                     float add_scale, float* dx, int64_t npix, int C, int eval, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(da && z && stats && dx && npix > 0 && C > 0 && (eval || sums), "disc_bn_bwd_dx: bad arguments");
  const long long total = (long long)npix * C;
  ONIRIS_CHECK_ARG((total + 255) / 256 <= 0x7fffffffLL, "disc_bn_bwd_dx: %lld elements", total);
  ONIRIS_KLAUNCH(disc_bn_bwd_dx_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, da, z, stats, sums,
                 add, add_scale, dx, total, C, 1.0f / (float)npix, eval);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}
