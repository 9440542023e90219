// Backward of the VAE at block widths above 64 channels (reference: edm2/vae/vae.py EncoderDecoder, :56-204), fp32 throughout,
// channels-last [B][T][H][W][C].  include/oniris.h: oniris_vae_wide_*_bwd.  The training forward is the inference launch sequence
// of csrc/vae_wide.hip without a cache.  Per wide ResBlock, out = x + b_B + convB(u), u = SiLU(RMS(a)), a = b_A + convA(S),
// S = [detach(y[:g]) ++ y], y = SiLU(RMS(x) (1 + scale) + shift):
//   oniris_vae_wide_act           S and u again (they are not stored)
//   oniris_vae_wide_conv_b_bwd    du = convB^T(dout): disc_conv_kernel on flipped, transposed weights
//   oniris_vae_wide_act_bwd       da from du (plain form), written in front of g zero frames: D = [da ++ 0]
//   oniris_vae_wide_conv_a        dy = convA^T(da): plane s of S is read by the output groups floor(s / g) - 1 and floor(s / g), so
//                                 d y of group tau reads frames tau g .. tau g + 2g - 1 of D -- the forward window -- on repacked weights;
//                                 what arrives on the g prefix planes of S is never formed (the prefix is detached)
//   oniris_vae_wide_act_bwd       dx from dy (FiLM form) + dout, and the per-workgroup partials of d scale | d shift
//   oniris_vae_wide_conv3_wgrad_bwd   the weight and bias gradients of conv A (2g g pairs of 9 taps) and conv B
// and the 1x1 stages: oniris_vae_wide_down_bwd (the adjoint of `down` and of `out`: vae_wide_kernel<NB, VW_UP> with Cin != Cout),
// oniris_vae_wide_up_bwd (the adjoint of `up`: vae_wide_down_kernel without the residual), oniris_vae_wide_lin_wgrad_bwd.
// Every sum has a fixed order set by the widths, g and the tile grid, nothing uses atomics, and a sample's activation gradients
// do not depend on B.
#include "oniris.h"
#include "common.h"
#include "vae_wide_train.h"

extern "C" int oniris_vae_wide_act_bwd(const float* x, const float* emb, const float* dy, const float* add, float* dx, float* part,
                                       int B, int T, int H, int W, int C, int out_T, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && dy && dx && dx != x && dx != dy, "vae_wide_act_bwd: null pointer or dx aliases an operand");
  ONIRIS_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && H > 0 && W > 0 && C > 0 && C <= 64 * VWT_NC_WIDE && out_T >= T,
                   "vae_wide_act_bwd: bad sizes (B %d T %d H %d W %d C %d out_T %d; C <= %d)", B, T, H, W, C, out_T, 64 * VWT_NC_WIDE);
  ONIRIS_CHECK_ARG(!part || emb, "vae_wide_act_bwd: partials of d scale | d shift without emb");
  const long long npix = (long long)T * H * W, P = (npix + VWT_PIX - 1) / VWT_PIX;
  ONIRIS_CHECK_ARG(P <= 0x7fffffffLL, "vae_wide_act_bwd: %lld pixels", npix);
  if (C <= 64 * VWT_NC)
    ONIRIS_KLAUNCH(vae_wide_act_bwd_kernel<VWT_NC>, dim3((unsigned)P, B), dim3(256), 0, (hipStream_t)stream, x, emb, dy, add, dx, part,
                   npix, (long long)out_T * H * W, C, B);
  else
    ONIRIS_KLAUNCH(vae_wide_act_bwd_kernel<VWT_NC_WIDE>, dim3((unsigned)P, B), dim3(256), 0, (hipStream_t)stream, x, emb, dy, add, dx,
                   part, npix, (long long)out_T * H * W, C, B);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_vae_wide_conv_b_bwd(const float* dout, const float* w, float* du, int B, int T, int H, int W, int C,
                                          oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(dout && w && du && du != dout, "vae_wide_conv_b_bwd: null pointer or du aliases dout");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && vae_wide_c_ok(C), "vae_wide_conv_b_bwd: bad sizes (B %d T %d H %d W %d C %d)", B,
                   T, H, W, C);
  return vae_wide_conv3_run("vae_wide_conv_b_bwd", dout, nullptr, w, nullptr, du, (long long)B * T, H, W, C, (hipStream_t)stream);
}

extern "C" int oniris_vae_wide_down_bwd(const float* dy, const float* w, const float* zero_bias, float* dx, int B, int T, int H, int W,
                                        int Cy, int Cx, int tcomp, int scomp, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(dy && w && zero_bias && dx && dx != dy, "vae_wide_down_bwd: null pointer or dx aliases dy");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && vae_wide_c_ok(Cy) && vae_wide_c_ok(Cx) && tcomp >= 1 && tcomp <= 2 &&
                       scomp >= 1 && scomp <= 2,
                   "vae_wide_down_bwd: bad sizes (B %d T %d H %d W %d Cy %d Cx %d tc %d sc %d)", B, T, H, W, Cy, Cx, tcomp, scomp);
  VaeWideParams p{};
  p.x = dy; p.w = w; p.bias = zero_bias; p.out = dx;
  p.B = B; p.T = T; p.H = H; p.W = W; p.Cin = Cy; p.Cout = Cx; p.nsub = tcomp * scomp * scomp; p.g = 1; p.tc = tcomp; p.sc = scomp;
  return vae_wide_dispatch<VW_UP>("vae_wide_down_bwd", p, (long long)B * T, (hipStream_t)stream);
}

extern "C" int oniris_vae_wide_up_bwd(const float* dup, const float* w, const float* zero_bias, float* dx, int B, int T, int H, int W,
                                      int C, int tcomp, int scomp, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(dup && w && zero_bias && dx && dx != dup, "vae_wide_up_bwd: null pointer or dx aliases dup");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && vae_wide_c_ok(C) && tcomp >= 1 && tcomp <= 2 && scomp >= 1 && scomp <= 2,
                   "vae_wide_up_bwd: bad sizes (B %d T %d H %d W %d C %d tc %d sc %d)", B, T, H, W, C, tcomp, scomp);
  VaeWideDownParams p{};
  p.x = dup; p.w = w; p.bias = zero_bias; p.out = dx;
  p.sc = 1; p.sw = C; p.sh = (long long)W * scomp * p.sw; p.st = (long long)H * scomp * p.sh; p.sb = (long long)T * tcomp * p.st;
  p.B = B; p.To = T; p.Ho = H; p.Wo = W; p.Cin = C; p.Cout = C; p.tc = tcomp; p.scm = scomp; p.normalize = 0;
  return vae_wide_down_run<false>("vae_wide_up_bwd", p, 0, (hipStream_t)stream);
}

template <typename K, typename P>
static int vae_wide_wgrad_launch(const char* what, K kern, const P& p, dim3 grid, hipStream_t stream) {
  const size_t bytes = ((size_t)DISC_HALO * DISC_HALO * DISC_WPITCH + 256 * 32) * sizeof(float);
  if (int rc = disc_raise_lds(kern, bytes, what)) return rc;
  ONIRIS_KLAUNCH(kern, grid, dim3(256), bytes, stream, p);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_vae_wide_conv3_wgrad_bwd(const float* xin, int x_T, const float* dA, int dA_T, int B, int T, int H, int W, int C,
                                               int g, int causal, float* slab, int nslab, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(xin && dA && slab && nslab > 0, "vae_wide_conv3_wgrad_bwd: null pointer or no slab");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && vae_wide_c_ok(C) && g >= 1 && g <= 8 && T % g == 0 && (causal || g == 1) &&
                       x_T >= T + (causal ? g : 0) && dA_T >= T,
                   "vae_wide_conv3_wgrad_bwd: bad sizes (B %d T %d H %d W %d C %d g %d causal %d, frames per sample %d / %d)", B, T, H,
                   W, C, g, causal, x_T, dA_T);
  VaeWideWgrad3Params p{};
  p.x = xin; p.dy = dA; p.slab = slab;
  p.ntau = T / g; p.g = g; p.KT = causal ? 2 * g : 1; p.xT = x_T; p.dyT = dA_T; p.H = H; p.W = W; p.C = C;
  p.tiles_x = cdiv(W, DISC_TILE); p.tiles_y = cdiv(H, DISC_TILE);
  const long long items = (long long)B * p.ntau * p.tiles_x * p.tiles_y;
  ONIRIS_CHECK_ARG(items <= 0x7fffffffLL && (long long)B * x_T <= 0x7fffffffLL && (long long)B * dA_T <= 0x7fffffffLL,
                   "vae_wide_conv3_wgrad_bwd: %lld work items", items);
  p.nitems = (int)items; p.nslab = nslab; p.ncib = cdiv(C, DISC_WKC);
  p.slab_size = (long long)p.KT * g * 9 * C * C + (long long)g * C;
  ONIRIS_CHECK_ARG((long long)p.KT * g * p.ncib <= 65535, "vae_wide_conv3_wgrad_bwd: %d pairs of %d channel blocks", p.KT * g, p.ncib);
  return vae_wide_wgrad_launch("vae_wide_conv3_wgrad_bwd", vae_wide_wgrad3_kernel, p, dim3(nslab, p.KT * g * p.ncib, cdiv(C, 32)),
                               (hipStream_t)stream);
}

extern "C" int oniris_vae_wide_lin_wgrad_bwd(const float* x, int64_t sb, int64_t st, int64_t sh, int64_t sw, int64_t sc, int Cx, int tcx,
                                             int scx, const float* dy, int Cy, int tcy, int scy, int B, int T, int H, int W,
                                             float* slab, int nslab, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && dy && slab && nslab > 0, "vae_wide_lin_wgrad_bwd: null pointer or no slab");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && vae_wide_c_ok(Cx) && vae_wide_c_ok(Cy) && tcx >= 1 && tcx <= 2 && scx >= 1 &&
                       scx <= 2 && tcy >= 1 && tcy <= 2 && scy >= 1 && scy <= 2,
                   "vae_wide_lin_wgrad_bwd: bad sizes (B %d T %d H %d W %d, views %d %d %d / %d %d %d)", B, T, H, W, Cx, tcx, scx, Cy,
                   tcy, scy);
  VaeWideWgrad1Params p{};
  p.x = x; p.dy = dy; p.slab = slab;
  p.xsb = sb; p.xst = st; p.xsh = sh; p.xsw = sw; p.xsc = sc;
  p.B = B; p.T = T; p.H = H; p.W = W; p.Cx = Cx; p.tcx = tcx; p.scx = scx; p.Cy = Cy; p.tcy = tcy; p.scy = scy;
  p.tiles_x = cdiv(W, DISC_TILE); p.tiles_y = cdiv(H, DISC_TILE);
  const long long items = (long long)B * T * p.tiles_x * p.tiles_y;
  ONIRIS_CHECK_ARG(items <= 0x7fffffffLL, "vae_wide_lin_wgrad_bwd: %lld work items", items);
  const int npairs = tcx * scx * scx * tcy * scy * scy;
  p.nitems = (int)items; p.nslab = nslab; p.ncib = cdiv(Cx, DISC_WKC);
  p.slab_size = (long long)npairs * Cx * Cy + (long long)tcy * scy * scy * Cy;
  ONIRIS_CHECK_ARG((long long)npairs * p.ncib <= 65535 && cdiv(Cy, 32) <= 65535, "vae_wide_lin_wgrad_bwd: %d pairs of %d channel blocks",
                   npairs, p.ncib);
  return vae_wide_wgrad_launch("vae_wide_lin_wgrad_bwd", vae_wide_wgrad1_kernel, p, dim3(nslab, npairs * p.ncib, cdiv(Cy, 32)),
                               (hipStream_t)stream);
}
