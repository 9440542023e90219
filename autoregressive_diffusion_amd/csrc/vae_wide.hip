// VAE decoder and encoder at block widths above 64 channels (reference: edm2/vae/vae.py EncoderDecoder, :56-204): inference, and
// the training forward (the backward is csrc/vae_wide_train.hip; the launch helpers both share are at the end of
// csrc/vae_wide_conv.h), fp32 throughout, channels-last [B][T][H][W][C].  include/oniris.h: oniris_vae_wide_*.  Per wide ResBlock:
//   oniris_vae_wide_temb    oniris_vae_temb for ResBlocks of any width (one launch per decode of a model with a wide block)
//   oniris_vae_wide_act     y = SiLU(RMS(x) (1 + scale) + shift) into the sequence buffer S = [g prefix frames ++ y] and the cache
//   oniris_vae_wide_conv_a  a = bias + the group-causal (2g, 3, 3) conv of S                (vae_wide_kernel<NB, VW_CONV_A>)
//   oniris_vae_wide_act     u = SiLU(RMS(a))
//   oniris_vae_wide_conv_b  out = res + bias + conv3x3(u)                                   (disc_conv_kernel<NB>, res_scale = 1)
// and the 1x1 stages as GEMMs on the same tile kernel: oniris_vae_wide_up, oniris_vae_wide_out (csrc/vae_wide_conv.h).
// The encoder at those widths runs the same ResBlock launches with a null emb (it passes t = None) behind oniris_vae_wide_down, the
// compression stage as a GEMM over the strided fp32 or uint8 input (vae_wide_down_kernel of csrc/vae_wide_conv.h).
// The convs take operands that are already activated: the cache is a plain copy of frames of S, and a conv of integers is exact.
// Nothing here bounds the width: VAE.max_width of autoregressive_diffusion_amd/vae.py does (256; VAE512: 512, where conv A of a
// block wider than 256 channels takes the 128-channel tile of vae_wide_nb_conv_a, csrc/vae_wide_conv.h).
#include "oniris.h"
#include "common.h"
#include "vae_conv3.h"
#include "disc_conv3.h"
#include "vae_wide_conv.h"

// ---- the activation pass: one wave per pixel, lane l holds channels l, l + 64, ...; the sum of squares is the lane's channels in
// ascending order, then the xor butterfly over the lanes -- an order that depends on C alone.
// Pixel p of S = [B][g + T][HW][C]: frame f < g is the prefix (a copy of cache_in; without one the workgroup of frame f + g
// writes it), frame f >= g is y of input frame f - g; the last g frames of S also go to cache_out.  g = 0: S = [B][T][HW][C].
__global__ __launch_bounds__(256) void vae_wide_act_kernel(const float* __restrict__ x, const float* __restrict__ emb,
                                                           const float* __restrict__ cache_in, float* __restrict__ cache_out,
                                                           float* __restrict__ S, long long total, int T, long long HW, int C, int g) {
  const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (p >= total) return;
  const long long q = p % HW, bf = p / HW;
  const int f = (int)(bf % (g + T));
  const long long b = bf / (g + T);
  float* dst = S + (size_t)p * C;
  if (f < g) {
    if (!cache_in) return;
    const float* src = cache_in + (((size_t)b * g + f) * HW + q) * C;
    for (int c = lane; c < C; c += 64) dst[c] = src[c];
    return;
  }
  const int t = f - g;
  const float* src = x + (((size_t)b * T + t) * HW + q) * C;
  const float* sc = emb ? emb + (size_t)b * 2 * C : nullptr;
  float ss = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float v = src[c];
    ss = fmaf(v, v, ss);
  }
  const float d = vae_rms(wave_sum(ss), C);
  float* pre = (!cache_in && t < g) ? S + (((size_t)b * (g + T) + t) * HW + q) * C : nullptr;
  float* co = (g > 0 && t >= T - g) ? cache_out + (((size_t)b * g + (t - (T - g))) * HW + q) * C : nullptr;
  for (int c = lane; c < C; c += 64) {
    const float v = vae_act(src[c], d, sc, C, c);
    dst[c] = v;
    if (pre) pre[c] = v;
    if (co) co[c] = v;
  }
}

// ---- t-embedding: vae_temb_kernel of csrc/vae.hip (the same operations in the same order, so the same bits) with the Fourier
// features of a ResBlock of any width in dynamic LDS; that kernel holds 128 of them, enough for 64 channels.
__global__ __launch_bounds__(128) void vae_wide_temb_kernel(const float* __restrict__ params, const int32_t* __restrict__ table,
                                                            const float* __restrict__ t, int B, float* __restrict__ emb) {
  extern __shared__ float vae_wide_f[];
  const int r = blockIdx.x, b = blockIdx.y;
  const int poff = table[3 * r], C2 = table[3 * r + 1], eoff = table[3 * r + 2] * B;
  const float* freqs = params + poff;
  const float* phases = freqs + C2;
  const float* W = phases + C2;
  const float* bias = W + (size_t)C2 * C2;
  const float tb = t[b];
  for (int k = threadIdx.x; k < C2; k += blockDim.x) vae_wide_f[k] = cosf(tb * freqs[k] + phases[k]) * 1.41421356237309515f;
  __syncthreads();
  for (int j = threadIdx.x; j < C2; j += blockDim.x) {
    float acc = 0.f;
    for (int k = 0; k < C2; ++k) acc = fmaf(W[(size_t)j * C2 + k], vae_wide_f[k], acc);
    emb[eoff + (size_t)b * C2 + j] = acc + bias[j];
  }
}

extern "C" int oniris_vae_wide_temb(const float* params, const int32_t* table, int n_res_blocks, int max_c2, const float* t, int B,
                                    float* emb, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(params && table && t && emb, "vae_wide_temb: null pointer");
  ONIRIS_CHECK_ARG(n_res_blocks > 0 && B > 0 && B <= 65535 && max_c2 > 0 && max_c2 <= 16384,
                   "vae_wide_temb: bad sizes (res blocks %d, B %d, widest 2C %d)", n_res_blocks, B, max_c2);
  ONIRIS_KLAUNCH(vae_wide_temb_kernel, dim3(n_res_blocks, B), dim3(128), (size_t)max_c2 * sizeof(float), (hipStream_t)stream, params,
                 table, t, B, emb);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_vae_wide_act(const float* x, const float* emb, const float* cache_in, float* cache_out, float* S, int B, int T,
                                   int H, int W, int C, int g, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && S && (const float*)S != x, "vae_wide_act: null pointer or S aliases x");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && vae_wide_c_ok(C) && g >= 0 && g <= 8,
                   "vae_wide_act: bad sizes (B %d T %d H %d W %d C %d g %d)", B, T, H, W, C, g);
  ONIRIS_CHECK_ARG(g == 0 ? (!cache_in && !cache_out) : (cache_out && T % g == 0 && cache_in != cache_out),
                   "vae_wide_act: g %d, T %d: the sequence form needs cache_out and T %% g == 0, the plain form no cache", g, T);
  const long long HW = (long long)H * W, total = (long long)B * (g + T) * HW;
  ONIRIS_CHECK_ARG((total + 3) / 4 <= 0x7fffffffLL, "vae_wide_act: %lld pixels", total);
  oniris_launch(vae_wide_act_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), (hipStream_t)stream, x, emb, cache_in, cache_out, S,
                total, T, HW, C, g);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_vae_wide_conv_a(const float* S, const float* w, const float* bias, float* out, int B, int T, int H, int W, int C,
                                      int g, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(S && w && bias && out && (const float*)out != S, "vae_wide_conv_a: null pointer or out aliases S");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && vae_wide_c_ok(C) && g >= 1 && g <= 8 && T % g == 0,
                   "vae_wide_conv_a: bad sizes (B %d T %d H %d W %d C %d g %d)", B, T, H, W, C, g);
  ONIRIS_CHECK_ARG((long long)B * (g + T) <= 0x7fffffffLL, "vae_wide_conv_a: %lld planes", (long long)B * (g + T));
  VaeWideParams p{};
  p.x = S; p.w = w; p.bias = bias; p.out = out;
  p.B = B; p.T = T; p.H = H; p.W = W; p.Cin = C; p.Cout = C; p.nsub = g; p.g = g;
  return vae_wide_dispatch<VW_CONV_A>("vae_wide_conv_a", p, (long long)B * (T / g), (hipStream_t)stream);
}

extern "C" int oniris_vae_wide_conv_b(const float* u, const float* res, const float* w, const float* bias, float* out, int B, int T,
                                      int H, int W, int C, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(u && res && w && bias && out && (const float*)out != u, "vae_wide_conv_b: null pointer or out aliases u");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && vae_wide_c_ok(C), "vae_wide_conv_b: bad sizes (B %d T %d H %d W %d C %d)", B, T,
                   H, W, C);
  return vae_wide_conv3_run("vae_wide_conv_b", u, res, w, bias, out, (long long)B * T, H, W, C, (hipStream_t)stream);
}

extern "C" int oniris_vae_wide_up(const float* x, const float* w, const float* bias, float* out, int B, int T, int H, int W, int C,
                                  int tcomp, int scomp, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && w && bias && out && (const float*)out != x, "vae_wide_up: null pointer or out aliases x");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && vae_wide_c_ok(C) && tcomp >= 1 && tcomp <= 2 && scomp >= 1 && scomp <= 2,
                   "vae_wide_up: bad sizes (B %d T %d H %d W %d C %d tc %d sc %d)", B, T, H, W, C, tcomp, scomp);
  VaeWideParams p{};
  p.x = x; p.w = w; p.bias = bias; p.out = out;
  p.B = B; p.T = T; p.H = H; p.W = W; p.Cin = C; p.Cout = C; p.nsub = tcomp * scomp * scomp; p.g = 1; p.tc = tcomp; p.sc = scomp;
  return vae_wide_dispatch<VW_UP>("vae_wide_up", p, (long long)B * T, (hipStream_t)stream);
}

extern "C" int oniris_vae_wide_out(const float* x, const float* w, const float* bias, int B, int T, int H, int W, int Cin, int Cout,
                                   int split, const float* logvar_mult, float* out, float* out2, int64_t sb, int64_t st, int64_t sh,
                                   int64_t sw, int64_t sc, uint8_t* frames, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && w && bias && (out || frames), "vae_wide_out: null pointer");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && vae_wide_c_ok(Cin) && vae_wide_c_ok(Cout) && split >= 0 && split < Cout,
                   "vae_wide_out: bad sizes (B %d T %d H %d W %d Cin %d Cout %d split %d)", B, T, H, W, Cin, Cout, split);
  ONIRIS_CHECK_ARG(split == 0 || (logvar_mult && (out2 || !out)), "vae_wide_out: the split needs logvar_mult and out2");
  ONIRIS_CHECK_ARG(!frames || split > 0, "vae_wide_out: frames need the mean / logvar split");
  VaeWideParams p{};
  p.x = x; p.w = w; p.bias = bias; p.out = out; p.out2 = out2; p.frames = (unsigned char*)frames; p.lvm = logvar_mult;
  p.B = B; p.T = T; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.nsub = 1; p.g = 1; p.split = split;
  p.sb = sb; p.st = st; p.sh = sh; p.sw = sw; p.scs = sc;
  return vae_wide_dispatch<VW_OUT>("vae_wide_out", p, (long long)B * T, (hipStream_t)stream);
}

extern "C" int oniris_vae_wide_down(const void* x, int x_is_u8, int64_t sb, int64_t st, int64_t sh, int64_t sw, int64_t sc, int B,
                                    int To, int Ho, int Wo, int Cin, int tcomp, int scomp, int normalize, const float* w,
                                    const float* bias, int Cout, float* out, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && w && bias && out && (const void*)out != x, "vae_wide_down: null pointer or out aliases x");
  ONIRIS_CHECK_ARG(B > 0 && To > 0 && Ho > 0 && Wo > 0 && vae_wide_c_ok(Cin) && vae_wide_c_ok(Cout) && tcomp >= 1 && tcomp <= 2 &&
                       scomp >= 1 && scomp <= 2,
                   "vae_wide_down: bad sizes (B %d T %d H %d W %d Cin %d tc %d sc %d Cout %d)", B, To, Ho, Wo, Cin, tcomp, scomp, Cout);
  VaeWideDownParams p{};
  p.x = x; p.w = w; p.bias = bias; p.out = out;
  p.sb = sb; p.st = st; p.sh = sh; p.sw = sw; p.sc = sc;
  p.B = B; p.To = To; p.Ho = Ho; p.Wo = Wo; p.Cin = Cin; p.Cout = Cout; p.tc = tcomp; p.scm = scomp; p.normalize = normalize;
  return vae_wide_down_run<true>("vae_wide_down", p, x_is_u8, (hipStream_t)stream);
}
