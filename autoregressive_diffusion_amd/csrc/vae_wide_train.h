// The backward kernels of the wide VAE (block widths above 64 channels) that the inference kernels do not already are: the
// activation adjoints and the weight gradients.  fp32, channels-last, 256 threads per workgroup.  The data gradients need no
// kernel of their own: they are vae_wide_kernel / vae_wide_down_kernel / disc_conv_kernel (csrc/vae_wide_conv.h) on repacked
// weights (csrc/vae_wide_train.hip says which).
//
//   vae_wide_act_bwd_kernel   one wave per pixel like vae_wide_act_kernel, lane l holds channels l, l + 64, ...: every channel sum is
//                             the lane's channels ascending, then the xor butterfly.  A workgroup walks VWT_PIX pixels of one sample
//                             (wave w takes w, w + 4, ...) and writes one partial of d scale | d shift.
//   vae_wide_wgrad3_kernel    weight and bias gradient of a ResBlock's convs on v_mfma_f32_32x32x2_f32, the walk of
//                             disc3d_wgrad_kernel over the parts of csrc/disc_parts.h: blockIdx.y carries the (time tap, frame in
//                             group) pair and the 32-channel block of Cin; workgroup s walks the work items (sample, group, tile) s,
//                             s + nslab, ... and writes slab s.  Any width: the last channel block is ragged.
//   vae_wide_wgrad1_kernel    the same at one tap for the 1x1 stages, both operands read through the rearranged views
//                             'b c (t tc) (h hc) (w wc) -> b (tc hc wc c) t h w'; blockIdx.y carries the pair of sub-positions.
#pragma once
#include "vae_conv3.h"
#include "vae_wide_conv.h"

#define VWT_PIX 256                                              // pixels per workgroup of the activation adjoint
#define VWT_NC 4                                                 // channels per lane there: widths up to 256
#define VWT_NC_WIDE 8                                            // and of the instantiation for widths up to 512

// y = SiLU(z), z = n (1 + scale) + shift, n = x / d, d = sqrt(mean_c x^2 + 1e-4) (emb NULL: z = n):
//   dz = dy SiLU'(z), dn = dz (1 + scale), dx = (dn - n mean_c(dn n)) / d (+ add), d scale = sum_pixels dz n, d shift = sum_pixels dz.
// x, dy, add [B][npix][C]; dx [B][out_npix][C] (pixels npix.. are the caller's); part [gridDim.x][B][2C] or NULL.
// NC: the channels a lane holds (C <= 64 NC); a lane's sums do not depend on it, so both instantiations give the same bits.
template <int NC>
__global__ __launch_bounds__(256) void vae_wide_act_bwd_kernel(const float* __restrict__ x, const float* __restrict__ emb,
                                                               const float* __restrict__ dy, const float* __restrict__ add,
                                                               float* __restrict__ dx, float* __restrict__ part, long long npix,
                                                               long long out_npix, int C, int B) {
  __shared__ float red[3][2 * NC * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
  const float* sc = emb ? emb + (size_t)b * 2 * C : nullptr;
  float ds[NC], dh[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) ds[i] = dh[i] = 0.f;
  for (int k = wave; k < VWT_PIX; k += 4) {
    const long long pp = (long long)blockIdx.x * VWT_PIX + k;
    if (pp >= npix) break;
    const size_t o = ((size_t)b * npix + pp) * C;
    float ss = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float v = x[o + c];
      ss = fmaf(v, v, ss);
    }
    const float d = vae_rms(wave_sum(ss), C);
    float dn[NC], xn[NC], m = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + 64 * i;
      dn[i] = xn[i] = 0.f;
      if (c < C) {
        const float n = x[o + c] / d;
        const float s1 = sc ? 1.f + sc[c] : 1.f;
        const float z = sc ? n * s1 + sc[C + c] : n;
        const float dz = dy[o + c] * vae_dsilu(z);
        dn[i] = dz * s1;
        xn[i] = n;
        m = fmaf(dn[i], n, m);
        if (part) {
          ds[i] = fmaf(dz, n, ds[i]);
          dh[i] += dz;
        }
      }
    }
    m = wave_sum(m) / (float)C;
    const size_t oo = ((size_t)b * out_npix + pp) * C;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + 64 * i;
      if (c < C) {
        float v = (dn[i] - xn[i] * m) / d;
        if (add) v += add[o + c];
        dx[oo + c] = v;
      }
    }
  }
  if (!part) return;
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      red[wave - 1][i * 64 + lane] = ds[i];
      red[wave - 1][(NC + i) * 64 + lane] = dh[i];
    }
  }
  __syncthreads();
  if (wave == 0) {
    float* o = part + ((size_t)blockIdx.x * B + b) * 2 * C;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + 64 * i;
      if (c < C) {
        float s = ds[i], h = dh[i];
        for (int w = 0; w < 3; ++w) {
          s += red[w][i * 64 + lane];
          h += red[w][(NC + i) * 64 + lane];
        }
        o[c] = s;
        o[C + c] = h;
      }
    }
  }
}

// x [B][xT][H][W][C], dy [B][dyT][H][W][C]; pair (kt, gl) of work item (n, tau): x plane n xT + tau g + kt, dy plane n dyT + tau g + gl.
// slab [KT][g][9][C][C] then the bias [g][C] (its owner: kt = 0, the first channel block).  Conv B: KT = g = 1.
struct VaeWideWgrad3Params {
  const float* x; const float* dy;
  float* slab;
  int ntau, g, KT, xT, dyT, H, W, C, tiles_x, tiles_y, nitems, nslab, ncib;
  long long slab_size;
};

__global__ __launch_bounds__(256) void vae_wide_wgrad3_kernel(VaeWideWgrad3Params p) {
  extern __shared__ __attribute__((aligned(16))) float disc_lds[];
  float* hl = disc_lds;                                          // [324][33]; afterwards the cross-wave sum [9][32][32]
  float* dyl = disc_lds + DISC_HALO * DISC_HALO * DISC_WPITCH;   // [256][32]; afterwards the bias sums [8][32]
  const int pair = blockIdx.y / p.ncib, ci0 = (blockIdx.y % p.ncib) * DISC_WKC, co0 = blockIdx.z * 32;
  const int kt = pair / p.g, gl = pair % p.g;
  const int kc = min(DISC_WKC, p.C - ci0);
  const int tiles = p.tiles_x * p.tiles_y;
  const bool bias_wg = kt == 0 && ci0 == 0;

  f32x16 acc[9];
  disc_zero(acc);
  float bsum = 0.f;
  for (int item = blockIdx.x; item < p.nitems; item += p.nslab) {
    const int pl = item / tiles, tile = item % tiles;            // pl = n ntau + tau
    const int n = pl / p.ntau, tau = pl % p.ntau;
    const int y0 = (tile / p.tiles_x) * DISC_TILE, x0 = (tile % p.tiles_x) * DISC_TILE;
    const int plane = n * p.xT + tau * p.g + kt;
    __syncthreads();
    if (p.C % 32 == 0) disc_stage_halo_vec<DISC_WPITCH, DISC_WKC>(hl, p.x, nullptr, nullptr, plane, y0, x0, p.H, p.W, p.C, ci0);
    else disc_stage_halo<DISC_WPITCH>(hl, p.x, nullptr, nullptr, plane, y0, x0, p.H, p.W, p.C, ci0, kc);
    disc_stage_dy(dyl, p.dy, n * p.dyT + tau * p.g + gl, y0, x0, p.H, p.W, p.C, co0);
    __syncthreads();
    disc_wgrad_mfma<9, 1, DISC_HALO, DISC_WPITCH>(acc, hl, dyl, kc);
    if (bias_wg) disc_bias_rows(bsum, dyl);
  }
  disc_wgrad_store<9>(acc, bsum, hl, dyl, p.slab + (size_t)blockIdx.x * p.slab_size, pair * 9, p.KT * p.g * 9, bias_wg, p.C, p.C, ci0,
                      co0, (size_t)gl * p.C);
}

// The 1x1 stages.  x: a tensor [B][T tcx][H scx][W scx][Cx] through element strides, dy: contiguous [B][T tcy][H scy][W scy][Cy];
// (B, T, H, W) the coarse grid.  pair = px npy + py of sub-positions pos = (tq sc + hq) sc + wq of x / dy.
// slab [npx][npy][Cx][Cy] then the bias [npy][Cy] (its owner: px = 0, the first channel block).
struct VaeWideWgrad1Params {
  const float* x; const float* dy;
  float* slab;
  long long xsb, xst, xsh, xsw, xsc;
  int B, T, H, W, Cx, tcx, scx, Cy, tcy, scy, tiles_x, tiles_y, nitems, nslab, ncib;
  long long slab_size;
};

// Channels co0 .. co0 + 31 of the tile's 256 pixels of one sub-position of dy (dys: the pixel (0, 0) of the plane at that
// sub-position; ysh / xsw: the strides of one coarse row / column) into dyl[256][32]; 0 outside.
__device__ __forceinline__ void vae_wide_stage_dy_view(float* dyl, const float* dys, long long ysh, long long xsw, int y0, int x0, int H,
                                                       int W, int Cy, int co0) {
  for (int idx = threadIdx.x; idx < 256 * 32; idx += 256) {
    const int co = idx & 31, pix = idx >> 5;
    const int y = y0 + (pix >> 4), xx = x0 + (pix & 15);
    float v = 0.f;
    if (y < H && xx < W && co0 + co < Cy) v = dys[y * ysh + xx * xsw + co0 + co];
    dyl[idx] = v;
  }
}

__global__ __launch_bounds__(256) void vae_wide_wgrad1_kernel(VaeWideWgrad1Params p) {
  extern __shared__ __attribute__((aligned(16))) float disc_lds[];
  float* hl = disc_lds;                                          // [324][33], the interior only; afterwards the cross-wave sum
  float* dyl = disc_lds + DISC_HALO * DISC_HALO * DISC_WPITCH;   // [256][32]; afterwards the bias sums [8][32]
  const int npy = p.tcy * p.scy * p.scy, npx = p.tcx * p.scx * p.scx;
  const int pair = blockIdx.y / p.ncib, ci0 = (blockIdx.y % p.ncib) * DISC_WKC, co0 = blockIdx.z * 32;
  const int px = pair / npy, py = pair % npy;
  const int kc = min(DISC_WKC, p.Cx - ci0);
  const int tiles = p.tiles_x * p.tiles_y;
  const bool bias_wg = px == 0 && ci0 == 0;
  const long long xoff = (px / (p.scx * p.scx)) * p.xst + ((px / p.scx) % p.scx) * p.xsh + (px % p.scx) * p.xsw;
  const long long dsw = p.Cy, dsh = (long long)p.W * p.scy * dsw, dst = (long long)p.H * p.scy * dsh;
  const long long yoff = (py / (p.scy * p.scy)) * dst + ((py / p.scy) % p.scy) * dsh + (py % p.scy) * dsw;

  f32x16 acc[1];
  disc_zero(acc);
  float bsum = 0.f;
  for (int item = blockIdx.x; item < p.nitems; item += p.nslab) {
    const int pl = item / tiles, tile = item % tiles;            // pl = n T + t
    const int n = pl / p.T, t = pl % p.T;
    const int y0 = (tile / p.tiles_x) * DISC_TILE, x0 = (tile % p.tiles_x) * DISC_TILE;
    const float* xs = p.x + n * p.xsb + (long long)t * p.tcx * p.xst + xoff;
    const float* dys = p.dy + ((long long)n * p.T + t) * p.tcy * dst + yoff;
    __syncthreads();
    vae_wide_stage_down<float, DISC_WPITCH>(hl, xs, p.scx * p.xsh, p.scx * p.xsw, p.xsc, 0, y0, x0, p.H, p.W, p.Cx, ci0, kc);
    vae_wide_stage_dy_view(dyl, dys, p.scy * dsh, p.scy * dsw, y0, x0, p.H, p.W, p.Cy, co0);
    __syncthreads();
    disc_wgrad_mfma<1, 1, DISC_HALO, DISC_WPITCH>(acc, hl, dyl, kc);
    if (bias_wg) disc_bias_rows(bsum, dyl);
  }
  disc_wgrad_store<1>(acc, bsum, hl, dyl, p.slab + (size_t)blockIdx.x * p.slab_size, pair, npx * npy, bias_wg, p.Cx, p.Cy, ci0, co0,
                      (size_t)py * p.Cy);
}
