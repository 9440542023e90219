// VAE training (reference: edm2/vae/vae.py VAE.forward :228-237 in training mode): the training forward of a ResBlock and the
// backward pass of every stage of the encoder and the decoder, fp32 throughout, channels-last [B][T][H][W][C] activations
// like the inference kernels (csrc/vae.hip, csrc/vae_encoder.hip), which the training forward also uses for its 1x1 stages.
//
// One tensor is saved per ResBlock beyond the block input x: a, the raw output of the group-causal conv.  Everything else is
// local to a pixel and recomputed while an operand is staged:  y = SiLU(RMS(x) (1 + scale) + shift)  and  u = SiLU(RMS(a)).
//   forward   oniris_vae_train_res_a   a = bias + conv_(2g,3,3)([detached first g frames of y] ++ y)        (vae.py:40-53)
//             oniris_vae_train_res_b   out = x + bias + conv_(3,3)(u)
//   backward  oniris_vae_res_b_bwd     da = adjoint of SiLU(RMS(.)) at a of  conv_(3,3)^T(dout)
//             oniris_vae_res_a_bwd     dx = dout + adjoint of SiLU(RMS(.)(1 + scale) + shift) at x of  conv_(2g,3,3)^T(da),
//                                      plus per-workgroup partial sums of d scale | d shift
//             oniris_vae_conv3_wgrad_bwd   weight and bias gradients of either conv into a bounded number of partial slabs
//             oniris_vae_lin_dx_bwd / oniris_vae_lin_dw_bwd   the 1x1 stages (down, up, out) seen as row-wise linear maps
//             oniris_vae_slab_sum_bwd  the sum of the slabs, slab 0 first
// No gradient flows through the time prefix (it is detached in the reference): frame f of y receives contributions from its own
// output group and from the next one only -- the causality of the forward mirrored, with a zero suffix in place of the prefix.
//
// Every sum has a fixed order and no floating-point atomic is used: two runs give bit-identical outputs and gradients.  The
// ResBlock's forward and data-gradient launches are vae_conv3_kernel<NCH, GPT, VT_FWD_A / VT_FWD_B / VT_DG_B / VT_DG_A> of
// csrc/vae_conv3.h, the kernel of the inference forward: staging, accumulation (time tap, row, column, input channel, then the
// bias) and activation are the same source, so the encoder's training forward is bit-identical to the inference one.
#include "vae_conv3.h"
#include "../../include/oniris.h"

// ---- weight and bias gradient of a 3x3 conv of a ResBlock.  dW[kt][gl][ky][kx][ci][c] = sum over b, tau, pixel of
// dA[frame tau g + gl][pixel][c] * in[frame(tau, kt)][pixel + (ky - 1, kx - 1)][ci] and db[gl][c] = sum dA, where `in` is the
// operand of the forward conv, recomputed while it is staged: SiLU(RMS(xin) (1 + scale) + shift).
//   causal = 1 (conv A): g output frames per group, KT = 2g taps, in frame(tau, kt) = f < g ? f : f - g with f = tau g + kt;
//   causal = 0 (conv B): g = 1, KT = 1, frame tau.
// Work item = (b, tau, 16x16 tile).  Workgroup s takes the items s, s + nslab, ... in that order and adds each item's sums over
// its 256 pixels (pixel order) into slab s, element e by the same thread every time: slab [nslab][KT g 9 C C + g C], zeroed by
// the caller.  A thread owns the elements e = tid + 256 i of the [9][ci][c] block of one (kt, gl), eight at a time in registers.
struct VtWgradParams {
  const float* xin;
  const float* emb;
  const float* dA;
  float* slab;
  int B, T, H, W, C, g, KT, causal, tiles_x, tiles_y, ntau, nitems, nslab;
  long long slab_size;
};

__global__ __launch_bounds__(256) void vt_wgrad3_kernel(VtWgradParams a) {
  extern __shared__ float smem[];
  const int C = a.C, H = a.H, W = a.W, T = a.T, g = a.g;
  const int CS = C | 1;
  float* tile = smem;                                        // [18 * 18][CS]  the activated operand with its halo
  float* dt = smem + VAE_HALO * VAE_HALO * CS;               // [256][C]       one frame of dA
  const int tid = threadIdx.x;
  const size_t frame = (size_t)H * W * C;
  const int NE = 9 * C * C;
  float* slab = a.slab + (size_t)blockIdx.x * a.slab_size;
  const int tiles = a.tiles_x * a.tiles_y;

  for (int item = blockIdx.x; item < a.nitems; item += a.nslab) {
    const int t_i = item % tiles;
    const int tau = (item / tiles) % a.ntau;
    const int b = item / (tiles * a.ntau);
    const int tx0 = (t_i % a.tiles_x) * VAE_TILE, ty0 = (t_i / a.tiles_x) * VAE_TILE;
    const float* sc = a.emb ? a.emb + (size_t)b * 2 * C : nullptr;
    for (int kt = 0; kt < a.KT; ++kt) {
      const int fp = a.causal ? tau * g + kt : tau;          // causal: a frame of the (prefix ++ input) sequence
      const int f = a.causal && fp >= g ? fp - g : fp;
      vae_stage_halo(tile, ty0, tx0, H, W, C, true, [&](float* dst, size_t pix, bool) {
        vae_activate(a.xin + ((size_t)b * T + f) * frame + pix, dst, C, sc, nullptr);
      });
      for (int gl = 0; gl < g; ++gl) {
        const int fo = a.causal ? tau * g + gl : tau;
        {
          const int y = ty0 + tid / VAE_TILE, xx = tx0 + tid % VAE_TILE;
          float* dst = dt + tid * C;
          if (y < H && xx < W) {
            const float* src = a.dA + ((size_t)b * T + fo) * frame + ((size_t)y * W + xx) * C;
            for (int c = 0; c < C; ++c) dst[c] = src[c];
          } else {
            for (int c = 0; c < C; ++c) dst[c] = 0.f;
          }
        }
        __syncthreads();
        if (kt == 0 && tid < C) {                            // the bias gradient, once per output frame
          float s = 0.f;
          for (int p = 0; p < 256; ++p) s += dt[p * C + tid];
          slab[(size_t)a.KT * g * NE + gl * C + tid] += s;
        }
        float* sl = slab + (size_t)(kt * g + gl) * NE;
        for (int e0 = tid; e0 < NE; e0 += 256 * 8) {
          float acc[8];
          int io[8], co[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int e = e0 + 256 * k < NE ? e0 + 256 * k : 0;
            const int kyx = e / (C * C), ci = (e / C) % C;
            co[k] = e % C;
            io[k] = ((kyx / 3) * VAE_HALO + kyx % 3) * CS + ci;
            acc[k] = 0.f;
          }
          const int nk = (NE - e0 + 255) / 256;              // how many of the eight exist for this thread
          for (int p = 0; p < 256; ++p) {
            const float* in = tile + ((p >> 4) * VAE_HALO + (p & 15)) * CS;
            const float* dd = dt + p * C;
#pragma unroll
            for (int k = 0; k < 8; ++k)
              if (k < nk) acc[k] = fmaf(in[io[k]], dd[co[k]], acc[k]);
          }
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (k < nk) sl[e0 + 256 * k] += acc[k];
        }
        __syncthreads();
      }
    }
  }
}

// ---- out[e] = slab[0][e] + slab[1][e] + ... in that order
__global__ __launch_bounds__(256) void vt_slab_sum_kernel(const float* __restrict__ slab, int nslab, long long n,
                                                          float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float s = 0.f;
  for (int i = 0; i < nslab; ++i) s += slab[(size_t)i * n + e];
  out[e] = s;
}

// ---- the 1x1 stages as linear maps over the rows of a coarse grid [B][T][H][W].  A "patch view" (C, tc, sc) of a channels-last
// tensor [B][T tc][H sc][W sc][C] is the matrix [row][pos C + c], pos = (tci sc + hci) sc + wci: the rearrangement of
// vae.py:157-164 (down: the view of the input; up: the view of the output; tc = sc = 1: the tensor itself).
struct VtView {
  int C, tc, sc;
};
__device__ __forceinline__ long long vt_view_off(long long row, int pos, int T, int H, int W, VtView v) {
  if (v.tc * v.sc == 1) return row * v.C;
  const int wc = pos % v.sc, hc = (pos / v.sc) % v.sc, tci = pos / (v.sc * v.sc);
  const int w = (int)(row % W);
  long long r = row / W;
  const int h = (int)(r % H); r /= H;
  const int t = (int)(r % T);
  const long long b = r / T;
  return ((((b * T + t) * v.tc + tci) * (long long)(H * v.sc) + h * v.sc + hc) * (long long)(W * v.sc) + w * v.sc + wc) * v.C;
}

// dx_view[row][k] = sum_n dy_view[row][n] * wc[n][k]  (n ascending), K = the columns of vx, N = those of vy
__global__ __launch_bounds__(256) void vt_lin_dx_kernel(const float* __restrict__ dy, VtView vy, const float* __restrict__ wc,
                                                        float* __restrict__ dx, VtView vx, int T, int H, int W, long long rows) {
  const int K = vx.C * vx.tc * vx.sc * vx.sc;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * K) return;
  const long long row = idx / K;
  const int k = (int)(idx % K);
  const int Py = vy.tc * vy.sc * vy.sc;
  float acc = 0.f;
  for (int pos = 0; pos < Py; ++pos) {
    const float* dp = dy + vt_view_off(row, pos, T, H, W, vy);
    const float* wr = wc + (size_t)pos * vy.C * K + k;
    for (int c = 0; c < vy.C; ++c) acc = fmaf(dp[c], wr[(size_t)c * K], acc);
  }
  dx[vt_view_off(row, k / vx.C, T, H, W, vx) + k % vx.C] = acc;
}

// dW[n][k] = sum_row dy_view[row][n] * x_view[row][k] for k < K and db[n] = dW[n][K] = sum_row dy_view[row][n].  Workgroup s
// takes the chunks of rpc rows s, s + nslab, ... in that order and adds each chunk's sums (row order) into slab s, element e
// by the same thread every time: slab [nslab][N][K + 1], zeroed by the caller.
__global__ __launch_bounds__(256) void vt_lin_dw_kernel(const float* __restrict__ x, VtView vx, const float* __restrict__ dy,
                                                        VtView vy, int T, int H, int W, long long rows, int rpc, int nslab,
                                                        float* __restrict__ slab_all) {
  extern __shared__ float smem[];
  const int K = vx.C * vx.tc * vx.sc * vx.sc, N = vy.C * vy.tc * vy.sc * vy.sc, K1 = K + 1;
  float* xs = smem;                                          // [rpc][K + 1], the last column 1 (0 beyond the last row)
  float* ys = smem + (size_t)rpc * K1;                       // [rpc][N]
  const int tid = threadIdx.x;
  const int NE = N * K1;
  float* slab = slab_all + (size_t)blockIdx.x * NE;
  for (long long r0 = (long long)blockIdx.x * rpc; r0 < rows; r0 += (long long)nslab * rpc) {
    for (int i = tid; i < rpc * K1; i += 256) {
      const int r = i / K1, k = i % K1;
      const long long row = r0 + r;
      float v = 0.f;
      if (row < rows) v = k == K ? 1.f : x[vt_view_off(row, k / vx.C, T, H, W, vx) + k % vx.C];
      xs[i] = v;
    }
    for (int i = tid; i < rpc * N; i += 256) {
      const int r = i / N, n = i % N;
      const long long row = r0 + r;
      ys[i] = row < rows ? dy[vt_view_off(row, n / vy.C, T, H, W, vy) + n % vy.C] : 0.f;
    }
    __syncthreads();
    for (int e0 = tid; e0 < NE; e0 += 256 * 8) {
      float acc[8];
      int xo[8], yo[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int e = e0 + 256 * k < NE ? e0 + 256 * k : 0;
        yo[k] = e / K1;
        xo[k] = e % K1;
        acc[k] = 0.f;
      }
      const int nk = (NE - e0 + 255) / 256;
      for (int r = 0; r < rpc; ++r) {
        const float* xr = xs + r * K1;
        const float* yr = ys + r * N;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k < nk) acc[k] = fmaf(yr[yo[k]], xr[xo[k]], acc[k]);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < nk) slab[e0 + 256 * k] += acc[k];
    }
    __syncthreads();
  }
}

// ---- host side
extern "C" int oniris_vae_train_res_a(const float* x, const float* emb, const float* w, const float* bias, int B, int T, int H,
                                      int W, int C, int g, int nch, int gpt, float* a_out, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && w && bias && a_out && (const float*)a_out != x, "vae_train_res_a: null or aliased pointer");
  VAE_CONV3_CHECK_GROUPED("vae_train_res_a");
  VaeConv3Params p{x, nullptr, nullptr, emb, w, bias, nullptr, nullptr, a_out, nullptr, T, H, W, C, g};
  return vae_conv3_dispatch<VT_FWD_A>("vae_train_res_a", p, B, nch, gpt, (hipStream_t)stream);
}

extern "C" int oniris_vae_train_res_b(const float* a_in, const float* res, const float* w, const float* bias, int B, int T,
                                      int H, int W, int C, int nch, float* out, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(a_in && res && w && bias && out && (const float*)out != a_in, "vae_train_res_b: null or aliased pointer");
  VAE_CONV3_CHECK_PLAIN("vae_train_res_b");
  VaeConv3Params p{a_in, nullptr, nullptr, nullptr, w, bias, res, nullptr, out, nullptr, T, H, W, C, 1};
  return vae_conv3_dispatch<VT_FWD_B>("vae_train_res_b", p, B, nch, 1, (hipStream_t)stream);
}

extern "C" int oniris_vae_res_b_bwd(const float* dout, const float* a_in, const float* wd, int B, int T, int H, int W, int C,
                                    int nch, float* da, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(dout && a_in && wd && da && (const float*)da != dout && (const float*)da != a_in,
                   "vae_res_b_bwd: null or aliased pointer");
  VAE_CONV3_CHECK_PLAIN("vae_res_b_bwd");
  VaeConv3Params p{dout, nullptr, nullptr, nullptr, wd, nullptr, a_in, nullptr, da, nullptr, T, H, W, C, 1};
  return vae_conv3_dispatch<VT_DG_B>("vae_res_b_bwd", p, B, nch, 1, (hipStream_t)stream);
}

extern "C" int oniris_vae_res_a_bwd(const float* da, const float* x, const float* emb, const float* dout, const float* wd, int B,
                                    int T, int H, int W, int C, int g, int nch, int gpt, float* dx, float* emb_part,
                                    oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(da && x && dout && wd && dx && (const float*)dx != da, "vae_res_a_bwd: null or aliased pointer");
  ONIRIS_CHECK_ARG(!emb_part || emb, "vae_res_a_bwd: emb_part without emb");
  VAE_CONV3_CHECK_GROUPED("vae_res_a_bwd");
  VaeConv3Params p{da, nullptr, nullptr, emb, wd, nullptr, x, dout, dx, emb_part, T, H, W, C, g};
  return vae_conv3_dispatch<VT_DG_A>("vae_res_a_bwd", p, B, nch, gpt, (hipStream_t)stream);
}

extern "C" int oniris_vae_conv3_wgrad_bwd(const float* xin, const float* emb, const float* dA, int B, int T, int H, int W, int C,
                                          int g, int causal, float* slab, int nslab, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(xin && dA && slab, "vae_conv3_wgrad_bwd: null pointer");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && C > 0 && C <= 64 && g >= 1 && (causal ? T % g == 0 : g == 1) && nslab > 0,
                   "vae_conv3_wgrad_bwd: bad sizes (B %d T %d H %d W %d C %d g %d causal %d nslab %d)", B, T, H, W, C, g, causal,
                   nslab);
  VtWgradParams p;
  p.xin = xin; p.emb = emb; p.dA = dA; p.slab = slab;
  p.B = B; p.T = T; p.H = H; p.W = W; p.C = C; p.g = g; p.KT = causal ? 2 * g : 1; p.causal = causal;
  p.tiles_x = cdiv(W, VAE_TILE); p.tiles_y = cdiv(H, VAE_TILE); p.ntau = causal ? T / g : T;
  const long long nitems = (long long)B * p.ntau * p.tiles_x * p.tiles_y;
  ONIRIS_CHECK_ARG(nitems <= 0x7fffffffLL, "vae_conv3_wgrad_bwd: %lld work items", nitems);
  p.nitems = (int)nitems;
  p.nslab = nslab;
  p.slab_size = (long long)p.KT * g * 9 * C * C + (long long)g * C;
  const size_t bytes = ((size_t)VAE_HALO * VAE_HALO * (C | 1) + (size_t)256 * C) * sizeof(float);
  if (int rc = vae_raise_lds<vt_wgrad3_kernel>(bytes, "vae_conv3_wgrad_bwd")) return rc;
  ONIRIS_KLAUNCH(vt_wgrad3_kernel, dim3(nslab), dim3(256), bytes, (hipStream_t)stream, p);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_vae_slab_sum_bwd(const float* slab, int nslab, int64_t n, float* out, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(slab && out && nslab > 0 && n > 0 && (n + 255) / 256 <= 0x7fffffffLL, "vae_slab_sum_bwd: bad arguments");
  oniris_launch(vt_slab_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), (hipStream_t)stream, slab, nslab, (long long)n,
                out);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

static bool vt_view_ok(int C, int tc, int sc) { return C > 0 && tc >= 1 && tc <= 2 && sc >= 1 && sc <= 2 && C * tc * sc * sc <= 512; }

extern "C" int oniris_vae_lin_dx_bwd(const float* dy, int Cy, int tcy, int scy, const float* wc, float* dx, int Cx, int tcx,
                                     int scx, int B, int T, int H, int W, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(dy && wc && dx, "vae_lin_dx_bwd: null pointer");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && vt_view_ok(Cy, tcy, scy) && vt_view_ok(Cx, tcx, scx),
                   "vae_lin_dx_bwd: bad sizes (B %d T %d H %d W %d, dy %d %d %d, dx %d %d %d)", B, T, H, W, Cy, tcy, scy, Cx, tcx,
                   scx);
  const long long rows = (long long)B * T * H * W;
  const long long total = rows * Cx * tcx * scx * scx;
  ONIRIS_CHECK_ARG((total + 255) / 256 <= 0x7fffffffLL, "vae_lin_dx_bwd: %lld threads", total);
  oniris_launch(vt_lin_dx_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), (hipStream_t)stream, dy, VtView{Cy, tcy, scy},
                wc, dx, VtView{Cx, tcx, scx}, T, H, W, rows);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

// rows per chunk of oniris_vae_lin_dw_bwd: what fits 48 KiB of LDS, between 8 and 128
static int vt_lin_rpc(int K, int N) {
  const int r = 12288 / (K + 1 + N);
  return r < 8 ? 8 : r > 128 ? 128 : r;
}

extern "C" int oniris_vae_lin_dw_bwd(const float* x, int Cx, int tcx, int scx, const float* dy, int Cy, int tcy, int scy, int B,
                                     int T, int H, int W, float* slab, int nslab, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && dy && slab && nslab > 0, "vae_lin_dw_bwd: null pointer");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && vt_view_ok(Cy, tcy, scy) && vt_view_ok(Cx, tcx, scx),
                   "vae_lin_dw_bwd: bad sizes (B %d T %d H %d W %d, x %d %d %d, dy %d %d %d)", B, T, H, W, Cx, tcx, scx, Cy, tcy,
                   scy);
  const int K = Cx * tcx * scx * scx, N = Cy * tcy * scy * scy;
  const int rpc = vt_lin_rpc(K, N);
  const size_t bytes = (size_t)rpc * (K + 1 + N) * sizeof(float);
  const long long rows = (long long)B * T * H * W;
  ONIRIS_KLAUNCH(vt_lin_dw_kernel, dim3(nslab), dim3(256), bytes, (hipStream_t)stream, x, VtView{Cx, tcx, scx}, dy,
                 VtView{Cy, tcy, scy}, T, H, W, rows, rpc, nslab, slab);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}
