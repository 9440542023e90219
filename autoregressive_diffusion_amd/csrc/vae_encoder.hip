// VAE encoder (reference: edm2/vae/vae.py EncoderDecoder(type='encoder') :96-204, VAE.encode :239-241), inference only,
// fp32 throughout: the way into and out of the ResBlocks.  The ResBlocks themselves are the decoder's oniris_vae_res_a /
// oniris_vae_res_b (csrc/vae.hip, csrc/vae_conv3.h) with a zero scale | shift buffer: the encoder passes t = None
// (vae.py:78-82) and v * (1 + 0) + 0 is exact.  Per encoder block one oniris_vae_down launch and two per ResBlock; one
// oniris_vae_latents launch at latent resolution per encode.
//
// Every output is summed in a fixed order (rearranged channel k ascending, then the bias, then the area residual) that
// depends on neither T, nor the batch, nor how a sequence was cut into chunks.
#include "common.h"
#include "../../include/oniris.h"

// one input element: fp32 as it is, uint8 converted exactly; normalize: frames / 127.5 - 1 (vae.py:271)
template <typename TIN>
__device__ __forceinline__ float vae_load_in(const TIN* p, int normalize) {
  const float v = (float)*p;
  return normalize ? __fsub_rn(__fdiv_rn(v, 127.5f), 1.f) : v;
}

// ---- down: 'b c (t tc) (h hc) (w wc) -> b (tc hc wc c) t h w' (vae.py:157-161), the compression 1x1 conv K = Cin tc sc^2
// -> Cout with bias, plus interpolate_channels of the rearranged input (F.interpolate mode='area' over the channel axis =
// adaptive average pooling, vae.py:109-122, :136-141; the index rule of vae_out_kernel), written channels-last.  The
// input is addressed through element strides.  One thread = one output pixel and four consecutive output channels: a
// wave's float4 stores cover 1 KiB of contiguous output.  The rearranged channels of one (tc, hc, wc) position are the
// Cin channels of one input pixel: read as float4 when VEC (fp32, unit channel stride, everything a multiple of 4).
// Every input value is read once and feeds both sums: w packed [K][2][G4] (G4 = Cout rounded up to 4) holds per rearranged
// channel k the conv weights and the 0 / 1 membership of k in the area window [floor(o K / Cout), ceil((o + 1) K / Cout))
// of every output o -- fma(1, v, a) and fma(0, v, a) are exact, so the window is summed in order k like vae_out_kernel
// does; bias packed [2][G4]: the bias and the window length.  out = (conv + bias) + window sum / window length.
template <typename TIN, bool VEC>
__global__ __launch_bounds__(256) void vae_down_kernel(const TIN* __restrict__ x, long long sb, long long st, long long sh,
                                                       long long sw, long long sc, int To, int Ho, int Wo, int Cin,
                                                       int tcomp, int scomp, int normalize, const float* __restrict__ w,
                                                       const float* __restrict__ bias, int Cout, long long total,
                                                       float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int G = (Cout + 3) / 4, G4 = 4 * G;
  const int o0 = (int)(idx % G) * 4;
  const long long pix = idx / G;
  long long p = pix;
  const int wo = (int)(p % Wo); p /= Wo;
  const int ho = (int)(p % Ho); p /= Ho;
  const int to = (int)(p % To);
  const long long b = p / To;
  const TIN* xb = x + b * sb + (long long)to * tcomp * st + (long long)ho * scomp * sh + (long long)wo * scomp * sw;
  const int P = tcomp * scomp * scomp;

  float acc[4] = {0.f, 0.f, 0.f, 0.f}, area[4] = {0.f, 0.f, 0.f, 0.f};
#define VAE_DOWN_FMA(v, wrow)                                                 \
  {                                                                           \
    const float4 wv = *(const float4*)(wrow), mv = *(const float4*)((wrow) + G4); \
    acc[0] = fmaf(wv.x, v, acc[0]); acc[1] = fmaf(wv.y, v, acc[1]);           \
    acc[2] = fmaf(wv.z, v, acc[2]); acc[3] = fmaf(wv.w, v, acc[3]);           \
    area[0] = fmaf(mv.x, v, area[0]); area[1] = fmaf(mv.y, v, area[1]);       \
    area[2] = fmaf(mv.z, v, area[2]); area[3] = fmaf(mv.w, v, area[3]);       \
  }
  for (int pos = 0; pos < P; ++pos) {
    const TIN* xp = xb + (long long)(pos / (scomp * scomp)) * st + (long long)((pos / scomp) % scomp) * sh +
                    (long long)(pos % scomp) * sw;
    const float* wr = w + (size_t)pos * Cin * 2 * G4 + o0;
    if (VEC) {
      for (int c = 0; c < Cin; c += 4) {
        const float4 v4 = *(const float4*)((const float*)xp + c);
        VAE_DOWN_FMA(v4.x, wr + (size_t)(c + 0) * 2 * G4)
        VAE_DOWN_FMA(v4.y, wr + (size_t)(c + 1) * 2 * G4)
        VAE_DOWN_FMA(v4.z, wr + (size_t)(c + 2) * 2 * G4)
        VAE_DOWN_FMA(v4.w, wr + (size_t)(c + 3) * 2 * G4)
      }
    } else {
      for (int c = 0; c < Cin; ++c) {
        const float v = vae_load_in(xp + c * sc, normalize);
        VAE_DOWN_FMA(v, wr + (size_t)c * 2 * G4)
      }
    }
  }
#undef VAE_DOWN_FMA

  const float4 bv = *(const float4*)(bias + o0), nv = *(const float4*)(bias + G4 + o0);
  const float r[4] = {(acc[0] + bv.x) + area[0] / nv.x, (acc[1] + bv.y) + area[1] / nv.y, (acc[2] + bv.z) + area[2] / nv.z,
                      (acc[3] + bv.w) + area[3] / nv.w};
  float* op = out + pix * Cout + o0;
  if ((Cout & 3) == 0) {
    *(float4*)op = make_float4(r[0], r[1], r[2], r[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (o0 + j < Cout) op[j] = r[j];
  }
}

// ---- latents: the last ResBlock's channels-last output [B][T][H][W][C] written through element strides, as it is
// (encode: (B, C, T, h, w)) or as (x - mean[c]) / std[c] (encode_frames: (B, T, C, h, w), the inverse of latents * std + mean
// of oniris_vae_up).  Threads run over the pixels of one channel: the stores follow the output's unit-stride width axis.
__global__ __launch_bounds__(256) void vae_latents_kernel(const float* __restrict__ x, int T, int H, int W, int C,
                                                          const float* __restrict__ mean, const float* __restrict__ std,
                                                          float* __restrict__ out, long long sb, long long st, long long sh,
                                                          long long sw, long long sc, long long npix) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= npix * C) return;
  const int c = (int)(idx / npix);
  const long long p = idx % npix;
  float v = x[p * C + c];
  if (mean) v = __fdiv_rn(__fsub_rn(v, mean[c]), std[c]);
  const int wq = (int)(p % W);
  long long q = p / W;
  const int hq = (int)(q % H); q /= H;
  const int tq = (int)(q % T);
  const long long bq = q / T;
  out[bq * sb + tq * st + hq * sh + wq * sw + (long long)c * sc] = v;
}

// ---- host side
extern "C" int oniris_vae_down(const void* x, int x_is_u8, int64_t sb, int64_t st, int64_t sh, int64_t sw, int64_t sc, int B,
                               int To, int Ho, int Wo, int Cin, int tcomp, int scomp, int normalize, const float* w,
                               const float* bias, int Cout, float* out, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && w && bias && out, "vae_down: null pointer");
  ONIRIS_CHECK_ARG(B > 0 && To > 0 && Ho > 0 && Wo > 0 && Cin > 0 && tcomp >= 1 && tcomp <= 2 && scomp >= 1 && scomp <= 2 &&
                       (long long)Cin * tcomp * scomp * scomp <= 512 && Cout > 0 && Cout <= 64,
                   "vae_down: bad sizes (B %d T %d H %d W %d Cin %d tc %d sc %d Cout %d)", B, To, Ho, Wo, Cin, tcomp, scomp, Cout);
  const long long total = (long long)B * To * Ho * Wo * ((Cout + 3) / 4);
  ONIRIS_CHECK_ARG((total + 255) / 256 <= 0x7fffffffLL, "vae_down: %lld threads", total);
  const dim3 grid((unsigned)((total + 255) / 256));
  hipStream_t s = (hipStream_t)stream;
#define VAE_DOWN_ARGS (long long)sb, (long long)st, (long long)sh, (long long)sw, (long long)sc, To, Ho, Wo, Cin, tcomp, scomp, \
                      normalize, w, bias, Cout, total, out
  if (x_is_u8) {
    oniris_launch((vae_down_kernel<unsigned char, false>), grid, dim3(256), s, (const unsigned char*)x, VAE_DOWN_ARGS);
  } else {
    const bool vec = !normalize && sc == 1 && Cin % 4 == 0 && sb % 4 == 0 && st % 4 == 0 && sh % 4 == 0 && sw % 4 == 0 &&
                     ((uintptr_t)x & 15) == 0;
    if (vec) oniris_launch((vae_down_kernel<float, true>), grid, dim3(256), s, (const float*)x, VAE_DOWN_ARGS);
    else oniris_launch((vae_down_kernel<float, false>), grid, dim3(256), s, (const float*)x, VAE_DOWN_ARGS);
  }
#undef VAE_DOWN_ARGS
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_vae_latents(const float* x, int B, int T, int H, int W, int C, const float* mean, const float* std,
                                  float* out, int64_t sb, int64_t st, int64_t sh, int64_t sw, int64_t sc,
                                  oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && out, "vae_latents: null pointer");
  ONIRIS_CHECK_ARG(!mean == !std, "vae_latents: mean and std go together");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && C > 0, "vae_latents: bad sizes (B %d T %d H %d W %d C %d)", B, T, H, W, C);
  const long long npix = (long long)B * T * H * W;
  oniris_launch(vae_latents_kernel, dim3((unsigned)((npix * C + 255) / 256)), dim3(256), (hipStream_t)stream, x, T, H, W, C, mean,
                std, out, (long long)sb, (long long)st, (long long)sh, (long long)sw, (long long)sc, npix);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}
