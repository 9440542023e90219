// VAE decoder (reference: edm2/vae/vae.py EncoderDecoder(type='decoder'), :56-204), inference only, fp32 throughout.
// Activations are channels-last [B][T][H][W][C] fp32, so that one pixel's channels are contiguous for the RMS norms.
// Per decoder block: oniris_vae_up (decompression 1x1 + 'up' rearrangement), per ResBlock oniris_vae_res_a (norm, FiLM,
// SiLU, group-causal (2g,3,3) conv, norm, SiLU) and oniris_vae_res_b (3x3 conv + residual), then oniris_vae_out (final 1x1 +
// channel-area residual; after the last block the mean / logvar split and, optionally, uint8 frames).  One
// oniris_vae_temb per decode computes the FiLM scale / shift of every ResBlock.  The two ResBlock launches are
// vae_conv3_kernel<NCH, GPT, VAE_RES_A / VAE_RES_B> of csrc/vae_conv3.h, which the training forward shares.
//
// Every output is summed in a fixed order (time tap, row, column, input channel, then the bias) that depends on neither
// T, nor the batch, nor how a sequence was cut into chunks: a streamed decode is bit-identical to the whole-sequence one.
#include "vae_conv3.h"
#include "../../include/oniris.h"

// ---- t-embedding: emb[r][b][j] = bias_r[j] + sum_k W_r[j][k] * sqrt(2) cos(t_b freq_r[k] + phase_r[k]), j < 2 C_r
// (MPFourier :139-150 of utils.py and ResBlock.t_cond, vae.py:76-80).  table[3 r .. 3 r + 2] = {parameter offset, 2 C_r,
// emb offset / B}; the parameters of block r are freqs[2C] | phases[2C] | W[2C][2C] | bias[2C].
__global__ __launch_bounds__(128) void vae_temb_kernel(const float* __restrict__ params, const int32_t* __restrict__ table,
                                                       const float* __restrict__ t, int B, float* __restrict__ emb) {
  __shared__ float f[128];
  const int r = blockIdx.x, b = blockIdx.y;
  const int poff = table[3 * r], C2 = table[3 * r + 1], eoff = table[3 * r + 2] * B;
  const float* freqs = params + poff;
  const float* phases = freqs + C2;
  const float* W = phases + C2;
  const float* bias = W + (size_t)C2 * C2;
  const float tb = t[b];
  for (int k = threadIdx.x; k < C2; k += blockDim.x) f[k] = cosf(tb * freqs[k] + phases[k]) * 1.41421356237309515f;
  __syncthreads();
  for (int j = threadIdx.x; j < C2; j += blockDim.x) {
    float acc = 0.f;
    for (int k = 0; k < C2; ++k) acc = fmaf(W[(size_t)j * C2 + k], f[k], acc);
    emb[eoff + (size_t)b * C2 + j] = acc + bias[j];
  }
}

// ---- up: the decompression 1x1 conv C -> C tc sc^2 (with bias) written straight to its 'b (tc hc wc c) t h w ->
// b c (t tc) (h hc) (w wc)' position (vae.py:96-133, :148-164).  The input is addressed through element strides (the
// latents of the first block arrive as (B, T, C, h, w) or (B, C, T, h, w)); in_scale / in_shift (or NULL) apply
// latents * std + mean per input channel first (latents_to_frames, vae.py:305).
__global__ __launch_bounds__(256) void vae_up_kernel(const float* __restrict__ x, long long sb, long long st, long long sh,
                                                     long long sw, long long sc, int T, int H, int W, int C,
                                                     const float* __restrict__ in_scale, const float* __restrict__ in_shift,
                                                     const float* __restrict__ w, const float* __restrict__ bias, int tcomp,
                                                     int scomp, long long total, float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int Wo = W * scomp, Ho = H * scomp, To = T * tcomp;
  const int c = (int)(idx % C);
  long long p = idx / C;
  const int wo = (int)(p % Wo); p /= Wo;
  const int ho = (int)(p % Ho); p /= Ho;
  const int to = (int)(p % To);
  const long long b = p / To;
  const int o = (((to % tcomp) * scomp + (ho % scomp)) * scomp + (wo % scomp)) * C + c;
  const float* xp = x + b * sb + (long long)(to / tcomp) * st + (long long)(ho / scomp) * sh + (long long)(wo / scomp) * sw;
  const float* wr = w + (size_t)o * C;
  float acc = 0.f;
  for (int ci = 0; ci < C; ++ci) {
    float v = xp[ci * sc];
    if (in_scale) v = __fmul_rn(v, in_scale[ci]) + in_shift[ci];
    acc = fmaf(wr[ci], v, acc);
  }
  out[idx] = acc + bias[o];
}

// ---- out: final 1x1 conv Cin -> Cout (with bias) + interpolate_channels(x, Cout) (F.interpolate mode='area' over the
// channel axis = adaptive average pooling, vae.py:136-141).  split > 0 (the last block): channels [0, split) go to out
// (mean), [split, Cout) to out2 (logvar, times exp(*logvar_mult)), both through element strides; frames (or NULL) receives
// uint8 clip((mean + 1) * 127.5, 0, 255) as [B][T][H][W][split] (latents_to_frames, vae.py:316-317); out NULL: frames only.
__global__ __launch_bounds__(256) void vae_out_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, int T, int H, int W, int Cin, int Cout,
                                                      int split, const float* __restrict__ logvar_mult, float* __restrict__ out,
                                                      float* __restrict__ out2, long long sb, long long st, long long sh,
                                                      long long sw, long long sc, unsigned char* __restrict__ frames,
                                                      long long npix, int chan_fastest) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= npix * Cout) return;
  const int o = chan_fastest ? (int)(idx % Cout) : (int)(idx / npix);
  const long long p = chan_fastest ? idx / Cout : idx % npix;
  const float* xp = x + p * Cin;
  const float* wr = w + (size_t)o * Cin;
  float acc = 0.f;
  for (int ci = 0; ci < Cin; ++ci) acc = fmaf(wr[ci], xp[ci], acc);
  const int s0 = (o * Cin) / Cout, s1 = ((o + 1) * Cin + Cout - 1) / Cout;
  float area = 0.f;
  for (int ci = s0; ci < s1; ++ci) area += xp[ci];
  float v = (acc + bias[o]) + area / (float)(s1 - s0);
  const int wq = (int)(p % W);
  long long q = p / W;
  const int hq = (int)(q % H); q /= H;
  const int tq = (int)(q % T);
  const long long bq = q / T;
  if (split > 0 && o >= split) {
    if (out) out2[bq * sb + tq * st + hq * sh + wq * sw + (long long)(o - split) * sc] = v * expf(*logvar_mult);
    return;
  }
  if (out) out[bq * sb + tq * st + hq * sh + wq * sw + (long long)o * sc] = v;
  if (frames) {
    float f = (v + 1.f) * 127.5f;
    f = fminf(fmaxf(f, 0.f), 255.f);
    frames[p * split + o] = (unsigned char)(int)f;
  }
}

// ---- host side
extern "C" int oniris_vae_temb(const float* params, const int32_t* table, int n_res_blocks, const float* t, int B, float* emb,
                               oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(params && table && t && emb, "vae_temb: null pointer");
  ONIRIS_CHECK_ARG(n_res_blocks > 0 && B > 0 && B <= 65535, "vae_temb: bad sizes (res blocks %d, B %d)", n_res_blocks, B);
  oniris_launch(vae_temb_kernel, dim3(n_res_blocks, B), dim3(128), (hipStream_t)stream, params, table, t, B, emb);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_vae_up(const float* x, int64_t sb, int64_t st, int64_t sh, int64_t sw, int64_t sc, int B, int T, int H,
                             int W, int C, const float* in_scale, const float* in_shift, const float* w, const float* bias,
                             int tcomp, int scomp, float* out, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && w && bias && out, "vae_up: null pointer");
  ONIRIS_CHECK_ARG(!in_scale == !in_shift, "vae_up: in_scale and in_shift go together");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && C > 0 && tcomp >= 1 && tcomp <= 2 && scomp >= 1 && scomp <= 2,
                   "vae_up: bad sizes (B %d T %d H %d W %d C %d tc %d sc %d)", B, T, H, W, C, tcomp, scomp);
  const long long total = (long long)B * T * tcomp * H * scomp * W * scomp * C;
  oniris_launch(vae_up_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), (hipStream_t)stream, x, (long long)sb,
                (long long)st, (long long)sh, (long long)sw, (long long)sc, T, H, W, C, in_scale, in_shift, w, bias, tcomp, scomp,
                total, out);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_vae_res_a(const float* x, const float* cache_in, float* cache_out, const float* emb, const float* w,
                                const float* bias, int B, int T, int H, int W, int C, int g, int nch, int gpt, float* out,
                                oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && cache_out && emb && w && bias && out, "vae_res_a: null pointer");
  ONIRIS_CHECK_ARG(cache_in != cache_out && (const float*)out != x, "vae_res_a: cache_out / out alias an input");
  VAE_CONV3_CHECK_GROUPED("vae_res_a");
  VaeConv3Params p{x, cache_in, cache_out, emb, w, bias, nullptr, nullptr, out, nullptr, T, H, W, C, g};
  return vae_conv3_dispatch<VAE_RES_A>("vae_res_a", p, B, nch, gpt, (hipStream_t)stream);
}

extern "C" int oniris_vae_res_b(const float* u, const float* res, const float* w, const float* bias, int B, int T, int H, int W,
                                int C, int nch, float* out, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(u && res && w && bias && out, "vae_res_b: null pointer");
  ONIRIS_CHECK_ARG((const float*)out != u, "vae_res_b: out aliases u");
  VAE_CONV3_CHECK_PLAIN("vae_res_b");
  VaeConv3Params p{u, nullptr, nullptr, nullptr, w, bias, res, nullptr, out, nullptr, T, H, W, C, 1};
  return vae_conv3_dispatch<VAE_RES_B>("vae_res_b", p, B, nch, 1, (hipStream_t)stream);
}

extern "C" int oniris_vae_out(const float* x, const float* w, const float* bias, int B, int T, int H, int W, int Cin, int Cout,
                              int split, const float* logvar_mult, float* out, float* out2, int64_t sb, int64_t st, int64_t sh,
                              int64_t sw, int64_t sc, uint8_t* frames, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && w && bias && (out || frames), "vae_out: null pointer");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && split >= 0 && split < Cout,
                   "vae_out: bad sizes (B %d T %d H %d W %d Cin %d Cout %d split %d)", B, T, H, W, Cin, Cout, split);
  ONIRIS_CHECK_ARG(split == 0 || (logvar_mult && (out2 || !out)), "vae_out: the split needs logvar_mult and out2");
  ONIRIS_CHECK_ARG(!frames || split > 0, "vae_out: frames need the mean / logvar split");
  const long long npix = (long long)B * T * H * W;
  const long long total = npix * Cout;
  oniris_launch(vae_out_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), (hipStream_t)stream, x, w, bias, T, H, W, Cin,
                Cout, split, logvar_mult, out, out2, (long long)sb, (long long)st, (long long)sh, (long long)sw, (long long)sc,
                (unsigned char*)frames, npix, (int)(sc == 1));
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}
