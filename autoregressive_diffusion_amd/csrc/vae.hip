// VAE decoder (reference: edm2/vae/vae.py EncoderDecoder(type='decoder'), :56-204), inference only, fp32 throughout.
// Activations are channels-last [B][T][H][W][C] fp32, so that one pixel's channels are contiguous for the RMS norms.
// Per decoder block: oniris_vae_up (decompression 1x1 + 'up' rearrangement), per ResBlock oniris_vae_res_a (norm, FiLM,
// SiLU, group-causal (2g,3,3) conv, norm, SiLU) and oniris_vae_res_b (3x3 conv + residual), then oniris_vae_out (final 1x1 +
// channel-area residual; after the last block the mean / logvar split and, optionally, uint8 frames).  One
// oniris_vae_temb per decode computes the FiLM scale / shift of every ResBlock.
//
// Every output is summed in a fixed order (time tap, row, column, input channel, then the bias) that depends on neither
// T, nor the batch, nor how a sequence was cut into chunks: a streamed decode is bit-identical to the whole-sequence one.
#include "common.h"
#include "../../include/oniris.h"

#define VAE_TILE 16
#define VAE_HALO (VAE_TILE + 2)
#define VAE_EPS 1e-4f

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

// ---- the two 3x3 convolutions of a ResBlock (vae.py:56-93).  One workgroup = a 16x16 pixel tile (one thread per pixel) of
// one output time step and one group of GPT output frames, every channel of them: the RMS norm of res A's epilogue is local
// to the thread.  Per time tap the activated input frame (with its one-pixel halo, zero outside the image) is staged in
// LDS, per stage of rows the packed weights; each input value read from LDS feeds NCH * GPT FMAs, each weight is a
// broadcast read.
//   MODE 0 (res A): out frame tau g + gq GPT + gl, channel c = SiLU(RMS(bias + sum_{kt < 2g, ky, kx, ci} w * a)), where a
//     is frame tau g + kt of [g prefix frames ++ the T input frames], each activated as SiLU(RMS(x) (1 + scale) + shift);
//     the prefix is the cache (already activated) or the first g input frames.  The workgroups of the last tau write the
//     activated last g input frames to cache_out.
//   MODE 1 (res B): out = res + bias + sum_{ky, kx, ci} w * u.
// Weights packed [T/g groups = g / GPT][KT][9][C][NCH * GPT], output j = c GPT + gl (c >= C: zero); bias [g / GPT][NCH GPT].
struct VaeConvParams {
  const float* x;          // MODE 0: block input [B][T][H][W][C]; MODE 1: res A output u
  const float* cache_in;   // MODE 0: [B][g][H][W][C] or NULL
  float* cache_out;        // MODE 0: [B][g][H][W][C]
  const float* emb;        // MODE 0: [B][2C] scale | shift
  const float* w;
  const float* bias;
  const float* res;        // MODE 1: residual [B][T][H][W][C]
  float* out;              // [B][T][H][W][C]
  int T, H, W, C, g, rows_per_stage, tiles_x, ngq;
};

template <int NCH, int GPT, int MODE>
__global__ __launch_bounds__(256) void vae_conv3_kernel(VaeConvParams a) {
  constexpr int NACC = NCH * GPT;
  extern __shared__ float smem[];
  const int C = a.C, H = a.H, W = a.W, T = a.T, g = a.g;
  const int CS = C | 1;                                      // odd pixel pitch: neighbouring pixels in different banks
  float* tile = smem;                                        // [18 * 18][CS]
  float* wsm = smem + VAE_HALO * VAE_HALO * CS;              // [rows_per_stage * 3][C][NACC]
  const int tid = threadIdx.x, px = tid % VAE_TILE, py = tid / VAE_TILE;
  const int tx0 = (blockIdx.x % a.tiles_x) * VAE_TILE, ty0 = (blockIdx.x / a.tiles_x) * VAE_TILE;
  const int b = blockIdx.z;
  const int tau = MODE == 0 ? (int)blockIdx.y / a.ngq : (int)blockIdx.y;
  const int gq = MODE == 0 ? (int)blockIdx.y % a.ngq : 0;
  const int KT = MODE == 0 ? 2 * g : 1;
  const size_t frame = (size_t)H * W * C;

  float acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j) acc[j] = 0.f;

  for (int kt = 0; kt < KT; ++kt) {
    // stage frame f of the (prefix ++ input) sequence, activated (MODE 0), with halo
    const int f = MODE == 0 ? tau * g + kt : tau;
    for (int p = tid; p < VAE_HALO * VAE_HALO; p += 256) {
      const int hy = p / VAE_HALO, hx = p % VAE_HALO;
      const int y = ty0 + hy - 1, xx = tx0 + hx - 1;
      float* dst = tile + p * CS;
      if (y < 0 || y >= H || xx < 0 || xx >= W) {
        for (int c = 0; c < C; ++c) dst[c] = 0.f;
        continue;
      }
      const size_t pix = ((size_t)y * W + xx) * C;
      if (MODE == 1) {
        const float* src = a.x + ((size_t)b * T + f) * frame + pix;
        for (int c = 0; c < C; ++c) dst[c] = src[c];
        continue;
      }
      if (f < g && a.cache_in) {
        const float* src = a.cache_in + ((size_t)b * g + f) * frame + pix;
        for (int c = 0; c < C; ++c) dst[c] = src[c];
        continue;
      }
      const float* src = a.x + ((size_t)b * T + (f < g ? f : f - g)) * frame + pix;
      float ss = 0.f;
      for (int c = 0; c < C; ++c) {
        const float v = src[c];
        dst[c] = v;
        ss = fmaf(v, v, ss);
      }
      const float d = sqrtf(ss / (float)C + VAE_EPS);
      const float* sc = a.emb + (size_t)b * 2 * C;
      float* co = (f >= T && gq == 0 && hy >= 1 && hy <= VAE_TILE && hx >= 1 && hx <= VAE_TILE)
                      ? a.cache_out + ((size_t)b * g + (f - T)) * frame + pix : nullptr;
      for (int c = 0; c < C; ++c) {
        float v = dst[c] / d;
        v = v * (1.f + sc[c]) + sc[C + c];
        v = v / (1.f + expf(-v));
        dst[c] = v;
        if (co) co[c] = v;
      }
    }
    for (int ky0 = 0; ky0 < 3; ky0 += a.rows_per_stage) {
      const int nw = a.rows_per_stage * 3 * C * NACC;        // a multiple of 4 (NACC >= 8)
      const float4* src = (const float4*)(a.w + (((size_t)gq * KT + kt) * 9 + ky0 * 3) * C * NACC);
      for (int i = tid; i < nw / 4; i += 256) ((float4*)wsm)[i] = src[i];
      __syncthreads();
      for (int kyl = 0; kyl < a.rows_per_stage; ++kyl)
        for (int kx = 0; kx < 3; ++kx) {
          const float* in = tile + ((py + ky0 + kyl) * VAE_HALO + px + kx) * CS;
          const float* wr = wsm + (kyl * 3 + kx) * C * NACC;
          for (int ci = 0; ci < C; ++ci) {
            const float v = in[ci];
            const float4* w4 = (const float4*)(wr + ci * NACC);
#pragma unroll
            for (int j4 = 0; j4 < NACC / 4; ++j4) {
              const float4 wv = w4[j4];
              acc[4 * j4 + 0] = fmaf(v, wv.x, acc[4 * j4 + 0]);
              acc[4 * j4 + 1] = fmaf(v, wv.y, acc[4 * j4 + 1]);
              acc[4 * j4 + 2] = fmaf(v, wv.z, acc[4 * j4 + 2]);
              acc[4 * j4 + 3] = fmaf(v, wv.w, acc[4 * j4 + 3]);
            }
          }
        }
      __syncthreads();
    }
  }

  const int y = ty0 + py, xx = tx0 + px;
  if (y >= H || xx >= W) return;
  const size_t pix = ((size_t)y * W + xx) * C;
  const float* bias = a.bias + (size_t)gq * NACC;
#pragma unroll
  for (int j = 0; j < NACC; ++j) acc[j] += bias[j];
  if (MODE == 1) {
    const float* r = a.res + ((size_t)b * T + tau) * frame + pix;
    float* o = a.out + ((size_t)b * T + tau) * frame + pix;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (c < C) o[c] = r[c] + acc[c];
    return;
  }
#pragma unroll
  for (int gl = 0; gl < GPT; ++gl) {
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (c < C) ss = fmaf(acc[c * GPT + gl], acc[c * GPT + gl], ss);
    const float d = sqrtf(ss / (float)C + VAE_EPS);
    float* o = a.out + ((size_t)b * T + (size_t)tau * g + gq * GPT + gl) * frame + pix;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (c < C) {
        const float v = acc[c * GPT + gl] / d;
        o[c] = v / (1.f + expf(-v));
      }
  }
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

template <int NCH, int GPT, int MODE>
static int vae_conv3_launch(const VaeConvParams& p, int B, int grid_y, hipStream_t stream) {
  constexpr int NACC = NCH * GPT;
  const size_t tile = (size_t)VAE_HALO * VAE_HALO * (p.C | 1) * sizeof(float);
  VaeConvParams a = p;
  a.rows_per_stage = tile + 9 * (size_t)p.C * NACC * sizeof(float) <= 64 * 1024 ? 3 : 1;
  const size_t bytes = tile + (size_t)a.rows_per_stage * 3 * p.C * NACC * sizeof(float);
  ONIRIS_CHECK_ARG(bytes <= 160 * 1024, "vae conv: %zu bytes of LDS", bytes);
  if (bytes > 64 * 1024) {
    static bool raised = false;
    if (!raised) {
      hipError_t e = hipFuncSetAttribute((const void*)vae_conv3_kernel<NCH, GPT, MODE>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (e != hipSuccess) {
        oniris_set_error("vae conv: raising the LDS limit failed: %s", hipGetErrorString(e));
        return ONIRIS_ELAUNCH;
      }
      raised = true;
    }
  }
  const dim3 grid(a.tiles_x * cdiv(p.H, VAE_TILE), grid_y, B);
  ONIRIS_KLAUNCH((vae_conv3_kernel<NCH, GPT, MODE>), grid, dim3(256), bytes, stream, a);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

// the (NCH, GPT) pairs that are instantiated: NCH in {8, 16, 32, 64} channels (C <= NCH), GPT output frames per thread with
// NCH * GPT <= 32 (64 for NCH = 64, GPT = 1)
#define VAE_CONV3_CASES(MODE)                                                         \
  if (nch == 8 && gpt == 1) return vae_conv3_launch<8, 1, MODE>(p, B, grid_y, s);     \
  if (nch == 8 && gpt == 2) return vae_conv3_launch<8, 2, MODE>(p, B, grid_y, s);     \
  if (nch == 8 && gpt == 4) return vae_conv3_launch<8, 4, MODE>(p, B, grid_y, s);     \
  if (nch == 16 && gpt == 1) return vae_conv3_launch<16, 1, MODE>(p, B, grid_y, s);   \
  if (nch == 16 && gpt == 2) return vae_conv3_launch<16, 2, MODE>(p, B, grid_y, s);   \
  if (nch == 32 && gpt == 1) return vae_conv3_launch<32, 1, MODE>(p, B, grid_y, s);   \
  if (nch == 64 && gpt == 1) return vae_conv3_launch<64, 1, MODE>(p, B, grid_y, s);

extern "C" int oniris_vae_res_a(const float* x, const float* cache_in, float* cache_out, const float* emb, const float* w,
                                const float* bias, int B, int T, int H, int W, int C, int g, int nch, int gpt, float* out,
                                oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && cache_out && emb && w && bias && out, "vae_res_a: null pointer");
  ONIRIS_CHECK_ARG(cache_in != cache_out && (const float*)out != x, "vae_res_a: cache_out / out alias an input");
  ONIRIS_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && C > 0 && C <= nch && g >= 1 && T >= g && T % g == 0 &&
                       gpt >= 1 && g % gpt == 0 && (long long)(T / g) * (g / gpt) <= 65535,
                   "vae_res_a: bad sizes (B %d T %d H %d W %d C %d g %d nch %d gpt %d)", B, T, H, W, C, g, nch, gpt);
  VaeConvParams p{x, cache_in, cache_out, emb, w, bias, nullptr, out, T, H, W, C, g, 3, cdiv(W, VAE_TILE), g / gpt};
  const int grid_y = (T / g) * (g / gpt);
  hipStream_t s = (hipStream_t)stream;
  VAE_CONV3_CASES(0)
  oniris_set_error("vae_res_a: no kernel for %d channels (capacity %d) with %d frames per thread", C, nch, gpt);
  return ONIRIS_EUNSUPPORTED;
}

extern "C" int oniris_vae_res_b(const float* u, const float* res, const float* w, const float* bias, int B, int T, int H, int W,
                                int C, int nch, float* out, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(u && res && w && bias && out, "vae_res_b: null pointer");
  ONIRIS_CHECK_ARG((const float*)out != u, "vae_res_b: out aliases u");
  ONIRIS_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && T <= 65535 && H > 0 && W > 0 && C > 0 && C <= nch,
                   "vae_res_b: bad sizes (B %d T %d H %d W %d C %d nch %d)", B, T, H, W, C, nch);
  VaeConvParams p{u, nullptr, nullptr, nullptr, w, bias, res, out, T, H, W, C, 1, 3, cdiv(W, VAE_TILE), 1};
  const int gpt = 1, grid_y = T;
  hipStream_t s = (hipStream_t)stream;
  VAE_CONV3_CASES(1)
  oniris_set_error("vae_res_b: no kernel for %d channels (capacity %d)", C, nch);
  return ONIRIS_EUNSUPPORTED;
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
