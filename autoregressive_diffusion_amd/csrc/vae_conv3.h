// The 3x3 tile kernel of the VAE's ResBlocks (reference: edm2/vae/vae.py :56-93), shared by inference (csrc/vae.hip) and training
// (csrc/vae_train.hip): the tile geometry, the per-pixel activation, the halo staging, the kernel with its weight stage and FMA
// loop, its launcher, the (NCH, GPT) dispatch and the argument checks.  fp32 throughout, channels-last [B][T][H][W][C].
//
// Every output is summed in a fixed order (time tap, row, column, input channel, then the bias) that depends on neither T, nor
// the batch, nor how a sequence was cut into chunks, and the training forward runs the staging, the accumulation and the bias of
// the inference forward: a streamed encode or decode is bit-identical to the whole-sequence one, and the encoder's training
// forward to the inference one.
#pragma once
#include "common.h"

#define VAE_TILE 16
#define VAE_HALO (VAE_TILE + 2)
#define VAE_EPS 1e-4f

// ---- the per-pixel activation SiLU(RMS(x) (1 + scale) + shift) over C channels: the RMS denominator from the sum of squares,
// one channel of it (sc = scale | shift, or NULL: SiLU(RMS(x))), and a whole pixel from src into dst and (unless NULL) copy
__device__ __forceinline__ float vae_rms(float ss, int C) { return sqrtf(ss / (float)C + VAE_EPS); }

__device__ __forceinline__ float vae_act(float v, float d, const float* sc, int C, int c) {
  v = v / d;
  if (sc) v = v * (1.f + sc[c]) + sc[C + c];
  return v / (1.f + expf(-v));
}

__device__ __forceinline__ void vae_activate(const float* src, float* dst, int C, const float* sc, float* copy) {
  float ss = 0.f;
  for (int c = 0; c < C; ++c) {
    const float v = src[c];
    dst[c] = v;
    ss = fmaf(v, v, ss);
  }
  const float d = vae_rms(ss, C);
  for (int c = 0; c < C; ++c) {
    const float v = vae_act(dst[c], d, sc, C, c);
    dst[c] = v;
    if (copy) copy[c] = v;
  }
}

__device__ __forceinline__ void vae_copy(const float* __restrict__ src, float* __restrict__ dst, int C) {
  for (int c = 0; c < C; ++c) dst[c] = src[c];
}

__device__ __forceinline__ float vae_dsilu(float v) {          // SiLU'(v) = s (1 + v (1 - s)), s = sigmoid(v)
  const float s = 1.f / (1.f + expf(-v));
  return s * (1.f + v * (1.f - s));
}

// ---- stage the 16x16 tile at (ty0, tx0) of one frame with its one-pixel halo into tile [18 * 18][C | 1] (odd pixel pitch:
// neighbouring pixels in different banks) by 256 threads: zeros outside the image (or everywhere: !live); a pixel inside gets
// pixel(dst, its offset in a [H][W][C] frame, whether it belongs to the tile proper)
template <class F>
__device__ __forceinline__ void vae_stage_halo(float* tile, int ty0, int tx0, int H, int W, int C, bool live, F pixel) {
  for (int p = threadIdx.x; p < VAE_HALO * VAE_HALO; p += 256) {
    const int hy = p / VAE_HALO, hx = p % VAE_HALO;
    const int y = ty0 + hy - 1, xx = tx0 + hx - 1;
    float* dst = tile + p * (C | 1);
    if (!live || y < 0 || y >= H || xx < 0 || xx >= W) {
      for (int c = 0; c < C; ++c) dst[c] = 0.f;
      continue;
    }
    pixel(dst, ((size_t)y * W + xx) * C, hy >= 1 && hy <= VAE_TILE && hx >= 1 && hx <= VAE_TILE);
  }
}

// ---- the kernel.  One workgroup = a 16x16 pixel tile (one thread per pixel) of one output time step and one group of GPT
// output frames, every channel of them in registers: the RMS norms of the epilogues are local to the thread.  Per time tap the
// operand frame (with its halo) is staged in LDS, per stage of rows the packed weights; each input value read from LDS feeds
// NCH * GPT FMAs, each weight is a broadcast read.  With y = SiLU(RMS(x) (1 + scale) + shift) and u = SiLU(RMS(a)):
//   VAE_RES_A  taps kt < 2g: frame tau g + kt of [g prefix frames ++ the T frames of y]; the prefix is cache_in (already
//              activated) or the first g frames of y; out: u of a = bias + conv, frames tau g + gq GPT + gl.  The workgroups of
//              the last tau write the last g frames of y to cache_out.
//   VAE_RES_B  one tap: frame tau of x = u; out = aux (the residual) + bias + conv
//   VT_FWD_A   VAE_RES_A without a cache; out: a itself
//   VT_FWD_B   VAE_RES_B with x = a, activated to u while it is staged
//   VT_DG_B    one tap: frame tau of x = dout; weights [9 flipped][co][ci]; out: da (aux = a)
//   VT_DG_A    taps j < 2g: frame q g + j of x = da (zero beyond T); weights [g / GPT][2g][9 flipped][c][ci GPT + rl] where tap
//              j < g is output frame gl = j of group q through time tap g + r, and tap j >= g is gl = j - g of group q + 1
//              through time tap r (r = gq GPT + rl, the position of the input frame inside its group); out: dx of frames q g + r
//              (aux = x, aux2 = dout); part (or NULL): [gridDim.y gridDim.x][B][2C] sums over the workgroup of d scale | d shift
// Forward weights packed [g / GPT][KT][9][C][NCH * GPT], output j = c GPT + gl (c >= C: zero); bias [g / GPT][NCH GPT].
enum { VAE_RES_A = 0, VAE_RES_B = 1, VT_FWD_A = 2, VT_FWD_B = 3, VT_DG_B = 4, VT_DG_A = 5 };
constexpr bool vae_conv3_grouped(int mode) { return mode == VAE_RES_A || mode == VT_FWD_A || mode == VT_DG_A; }

struct VaeConv3Params {
  const float* x;          // the operand [B][T][H][W][C]
  const float* cache_in;   // VAE_RES_A: [B][g][H][W][C] or NULL
  float* cache_out;        // VAE_RES_A: [B][g][H][W][C]
  const float* emb;        // [B][2C] scale | shift (training: or NULL)
  const float* w;
  const float* bias;
  const float* aux;
  const float* aux2;
  float* out;              // [B][T][H][W][C]
  float* part;
  int T, H, W, C, g, rows_per_stage, tiles_x, ngq;
};

template <int NCH, int GPT, int MODE>
__global__ __launch_bounds__(256) void vae_conv3_kernel(VaeConv3Params a) {
  constexpr int NACC = NCH * GPT;
  constexpr bool GROUPED = vae_conv3_grouped(MODE);
  constexpr bool PREFIXED = MODE == VAE_RES_A || MODE == VT_FWD_A;
  extern __shared__ float smem[];
  const int C = a.C, H = a.H, W = a.W, T = a.T, g = a.g;
  const int CS = C | 1;
  float* tile = smem;                                        // [18 * 18][CS]
  float* wsm = smem + VAE_HALO * VAE_HALO * CS;              // [rows_per_stage * 3][C][NACC]
  const int tid = threadIdx.x, px = tid % VAE_TILE, py = tid / VAE_TILE;
  const int tx0 = (blockIdx.x % a.tiles_x) * VAE_TILE, ty0 = (blockIdx.x / a.tiles_x) * VAE_TILE;
  const int b = blockIdx.z;
  const int tau = GROUPED ? (int)blockIdx.y / a.ngq : (int)blockIdx.y;
  const int gq = GROUPED ? (int)blockIdx.y % a.ngq : 0;
  const int KT = GROUPED ? 2 * g : 1;
  const size_t frame = (size_t)H * W * C;
  const float* sc = a.emb ? a.emb + (size_t)b * 2 * C : nullptr;
  if (MODE == VAE_RES_A) __builtin_assume(sc != nullptr);    // oniris_vae_res_a refuses a NULL emb: no test per channel

  float acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j) acc[j] = 0.f;

  for (int kt = 0; kt < KT; ++kt) {
    const int f = GROUPED ? tau * g + kt : tau;              // PREFIXED: a frame of the (prefix ++ input) sequence
    vae_stage_halo(tile, ty0, tx0, H, W, C, MODE != VT_DG_A || f < T, [&](float* dst, size_t pix, bool inner) {
      if (MODE == VAE_RES_A && f < g && a.cache_in) {
        vae_copy(a.cache_in + ((size_t)b * g + f) * frame + pix, dst, C);
        return;
      }
      const float* src = a.x + ((size_t)b * T + (PREFIXED && f >= g ? f - g : f)) * frame + pix;
      if (PREFIXED) {
        const bool keep = MODE == VAE_RES_A && f >= T && gq == 0 && inner;
        vae_activate(src, dst, C, sc, keep ? a.cache_out + ((size_t)b * g + (f - T)) * frame + pix : nullptr);
      } else if (MODE == VT_FWD_B) {
        vae_activate(src, dst, C, nullptr, nullptr);
      } else {
        vae_copy(src, dst, C);
      }
    });
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
  const bool inside = y < H && xx < W;
  const size_t pix = inside ? ((size_t)y * W + xx) * C : 0;

  if (MODE != VT_DG_A && !inside) return;                    // VT_DG_A: no thread leaves before the wave sums
  if (MODE != VT_DG_B && MODE != VT_DG_A) {
    const float* bias = a.bias + (size_t)gq * NACC;
#pragma unroll
    for (int j = 0; j < NACC; ++j) acc[j] += bias[j];
  }
  if (MODE == VAE_RES_B || MODE == VT_FWD_B) {
    const float* r = a.aux + ((size_t)b * T + tau) * frame + pix;
    float* o = a.out + ((size_t)b * T + tau) * frame + pix;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (c < C) o[c] = r[c] + acc[c];
    return;
  }
  if (PREFIXED) {
#pragma unroll
    for (int gl = 0; gl < GPT; ++gl) {
      float d = 0.f;
      if (MODE == VAE_RES_A) {
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
          if (c < C) ss = fmaf(acc[c * GPT + gl], acc[c * GPT + gl], ss);
        d = vae_rms(ss, C);
      }
      float* o = a.out + ((size_t)b * T + (size_t)tau * g + gq * GPT + gl) * frame + pix;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
        if (c < C) o[c] = MODE == VAE_RES_A ? vae_act(acc[c * GPT + gl], d, nullptr, C, c) : acc[c * GPT + gl];
    }
    return;
  }

  if (MODE == VT_DG_B) {                                     // acc = du; da = (dr - r mean(dr r)) / d, dr = du SiLU'(r), r = a / d
    const float* ap = a.aux + ((size_t)b * T + tau) * frame + pix;
    float* o = a.out + ((size_t)b * T + tau) * frame + pix;
    float ss = 0.f;
    for (int c = 0; c < C; ++c) ss = fmaf(ap[c], ap[c], ss);
    const float d = vae_rms(ss, C);
    float m = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (c < C) {
        const float r = ap[c] / d;
        acc[c] *= vae_dsilu(r);
        m = fmaf(acc[c], r, m);
      }
    m /= (float)C;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (c < C) o[c] = (acc[c] - (ap[c] / d) * m) / d;
    return;
  }

  // VT_DG_A: acc[ci GPT + rl] = dy of frame q g + gq GPT + rl.  With n = x / d, v = n (1 + scale) + shift:  dv = dy SiLU'(v),
  // d scale += dv n, d shift += dv, dn = dv (1 + scale), dx = (dn - n mean(dn n)) / d + dout.  A pixel outside the image
  // contributes zero to the wave sums.
  float* red = smem;                                         // [4 waves][2C], free after the last barrier of the loop
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int rl = 0; rl < GPT; ++rl) {
    const size_t off = ((size_t)b * T + (size_t)tau * g + gq * GPT + rl) * frame + pix;
    const float* xp = a.aux + off;
    float ss = 0.f;
    if (inside)
      for (int c = 0; c < C; ++c) ss = fmaf(xp[c], xp[c], ss);
    const float d = vae_rms(ss, C);
    float m = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (c < C) {
        float dv = 0.f, n = 0.f, s1 = 0.f;
        if (inside) {
          n = xp[c] / d;
          s1 = sc ? 1.f + sc[c] : 1.f;
          const float v = sc ? n * s1 + sc[C + c] : n;
          dv = acc[c * GPT + rl] * vae_dsilu(v);
        }
        const float dn = dv * s1;
        acc[c * GPT + rl] = dn;
        m = fmaf(dn, n, m);
        if (a.part) {
          const float ps = wave_sum(dv * n), ph = wave_sum(dv);
          if (lane == 0) {
            red[wave * 2 * C + c] = (rl == 0 ? 0.f : red[wave * 2 * C + c]) + ps;
            red[wave * 2 * C + C + c] = (rl == 0 ? 0.f : red[wave * 2 * C + C + c]) + ph;
          }
        }
      }
    m /= (float)C;
    if (inside) {
      const float* go = a.aux2 + off;
      float* o = a.out + off;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
        if (c < C) o[c] = (acc[c * GPT + rl] - (xp[c] / d) * m) / d + go[c];
    }
  }
  if (a.part) {
    __syncthreads();
    if (tid < 2 * C) {
      const float s = ((red[tid] + red[2 * C + tid]) + red[4 * C + tid]) + red[6 * C + tid];
      a.part[(((size_t)blockIdx.y * gridDim.x + blockIdx.x) * gridDim.z + b) * 2 * C + tid] = s;
    }
  }
}

// ---- host side.  A launch that needs more than the default 64 KiB of dynamic LDS raises KERNEL's limit to the 160 KiB of a
// gfx950 CU first, once per kernel.
template <auto KERNEL>
static int vae_raise_lds(size_t bytes, const char* what) {
  static bool raised = false;
  if (bytes <= 64 * 1024 || raised) return ONIRIS_OK;
  hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) {
    oniris_set_error("%s: raising the LDS limit failed: %s", what, hipGetErrorString(e));
    return ONIRIS_ELAUNCH;
  }
  raised = true;
  return ONIRIS_OK;
}

// The weights of all three rows are staged at once when they fit the default 64 KiB next to the tile, else row by row.
template <int NCH, int GPT, int MODE>
static int vae_conv3_launch(VaeConv3Params a, int B, hipStream_t stream) {
  constexpr int NACC = NCH * GPT;
  const char* what = MODE == VAE_RES_A || MODE == VAE_RES_B ? "vae conv" : "vae training conv";
  const size_t tile = (size_t)VAE_HALO * VAE_HALO * (a.C | 1) * sizeof(float);
  a.rows_per_stage = tile + 9 * (size_t)a.C * NACC * sizeof(float) <= 64 * 1024 ? 3 : 1;
  a.tiles_x = cdiv(a.W, VAE_TILE);
  a.ngq = a.g / GPT;
  const size_t bytes = tile + (size_t)a.rows_per_stage * 3 * a.C * NACC * sizeof(float);
  ONIRIS_CHECK_ARG(bytes <= 160 * 1024, "%s: %zu bytes of LDS", what, bytes);
  if (int rc = vae_raise_lds<vae_conv3_kernel<NCH, GPT, MODE>>(bytes, what)) return rc;
  const dim3 grid(a.tiles_x * cdiv(a.H, VAE_TILE), vae_conv3_grouped(MODE) ? (a.T / a.g) * a.ngq : a.T, B);
  ONIRIS_KLAUNCH((vae_conv3_kernel<NCH, GPT, MODE>), grid, dim3(256), bytes, stream, a);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

// The (NCH, GPT) pairs that are instantiated: NCH in {8, 16, 32, 64} channels (C <= NCH), GPT output frames per thread with
// NCH * GPT <= 32 (64 for NCH = 64, GPT = 1); a mode without frame groups takes the pairs with GPT = 1.
template <int MODE>
static int vae_conv3_dispatch(const char* what, const VaeConv3Params& p, int B, int nch, int gpt, hipStream_t stream) {
#define VAE_CONV3_CASE(NCH, GPT)                       \
  if constexpr (GPT == 1 || vae_conv3_grouped(MODE))   \
    if (nch == NCH && gpt == GPT) return vae_conv3_launch<NCH, GPT, MODE>(p, B, stream);
  VAE_CONV3_CASE(8, 1) VAE_CONV3_CASE(8, 2) VAE_CONV3_CASE(8, 4) VAE_CONV3_CASE(16, 1) VAE_CONV3_CASE(16, 2)
  VAE_CONV3_CASE(32, 1) VAE_CONV3_CASE(64, 1)
#undef VAE_CONV3_CASE
  if (vae_conv3_grouped(MODE))
    oniris_set_error("%s: no kernel for %d channels (capacity %d) with %d frames per thread", what, p.C, nch, gpt);
  else
    oniris_set_error("%s: no kernel for %d channels (capacity %d)", what, p.C, nch);
  return ONIRIS_EUNSUPPORTED;
}

// the size checks of an entry point with frame groups (B, T, H, W, C, g, nch, gpt in scope) and of one without (no g, gpt)
#define VAE_CONV3_CHECK_GROUPED(what)                                                                                     \
  ONIRIS_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && C > 0 && C <= nch && g >= 1 && T >= g && T % g == 0 &&        \
                       gpt >= 1 && g % gpt == 0 && (long long)(T / g) * (g / gpt) <= 65535,                               \
                   what ": bad sizes (B %d T %d H %d W %d C %d g %d nch %d gpt %d)", B, T, H, W, C, g, nch, gpt)
#define VAE_CONV3_CHECK_PLAIN(what)                                                                        \
  ONIRIS_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && T <= 65535 && H > 0 && W > 0 && C > 0 && C <= nch,      \
                   what ": bad sizes (B %d T %d H %d W %d C %d nch %d)", B, T, H, W, C, nch)
