// The wide VAE's inference convs on bf16 MFMA operands: the entry points oniris_vae_wide_{conv_a, conv_b, up, out, down}_bf16 of
// include/oniris.h over the kernels of csrc/vae_wide_bf16.h (the numerical contract is stated there).  Each has the arguments,
// the checks and the error codes of its fp32 sibling in csrc/vae_wide.hip; w holds bf16 bit patterns in the sibling's layout with
// CinP = Cin rounded up to a multiple of 16.  The activation pass and the t-embedding stay oniris_vae_wide_act / _temb.
#include "oniris.h"
#include "common.h"
#include "vae_wide_bf16.h"

static inline bool vbf_aligned(const void* p, int n) { return ((uintptr_t)p & (n - 1)) == 0; }

template <int NB, int MODE>
static int vbf_launch(const char* what, const VaeWideBf16Params& q, dim3 grid, hipStream_t stream) {
  constexpr int TAPS = (MODE == VW_CONV_A || MODE == VBF_CONV_B) ? 9 : 1;
  const size_t bytes = ((size_t)DISC_HALO * DISC_HALO + (size_t)TAPS * 32 * NB) * VBF_PITCH * sizeof(bf16);
  if (int rc = disc_raise_lds(vae_wide_bf16_kernel<NB, MODE>, bytes, what)) return rc;
  ONIRIS_KLAUNCH((vae_wide_bf16_kernel<NB, MODE>), grid, dim3(256), bytes, stream, q);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

// planes: the output planes a workgroup column walks; q.p.nsub, Cin, Cout, H, W set.  64 output channels per workgroup where the
// padded width allows, else 32 (vae_wide_nb), for every stage: conv A's 128-channel tile of the fp32 path (vae_wide_nb_conv_a)
// was measured here too and lost 26 % at C = 512, g = 4 (one workgroup per CU instead of two: profiles/vae_bf16.txt).
template <int MODE>
static int vbf_dispatch(const char* what, VaeWideBf16Params& q, long long planes, hipStream_t stream) {
  VaeWideParams& p = q.p;
  ONIRIS_CHECK_ARG(vbf_aligned(q.w, 4), "%s: w must be 4-byte aligned", what);
  p.CinP = roundup(p.Cin, VBF_KSTEP);
  p.CP = roundup(p.Cout, 32);
  p.tiles_x = cdiv(p.W, DISC_TILE); p.tiles_y = cdiv(p.H, DISC_TILE);
  q.vec = p.Cin % 8 == 0 && vbf_aligned(p.x, 16);
  const int nb = vae_wide_nb(p.CP);
  p.nblk = p.CP / (32 * nb);
  const long long wgs = planes * p.tiles_x * p.tiles_y;
  ONIRIS_CHECK_ARG(planes <= 0x7fffffffLL && wgs <= 0x7fffffffLL && (long long)p.nsub * p.nblk <= 65535, "%s: %lld tiles", what, wgs);
  const dim3 grid((unsigned)wgs, p.nsub * p.nblk);
  return nb == 2 ? vbf_launch<2, MODE>(what, q, grid, stream) : vbf_launch<1, MODE>(what, q, grid, stream);
}

template <int NB, typename TIN, bool VEC>
static int vbf_down_launch(const char* what, const VaeWideDownBf16Params& q, dim3 grid, hipStream_t stream) {
  const size_t bytes = ((size_t)DISC_HALO * DISC_HALO + (size_t)32 * NB) * VBF_PITCH * sizeof(bf16);
  ONIRIS_KLAUNCH((vae_wide_down_bf16_kernel<NB, TIN, VEC>), grid, dim3(256), bytes, stream, q);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

template <int NB>
static int vbf_down_pick(const char* what, const VaeWideDownBf16Params& q, int x_is_u8, bool vec, dim3 grid, hipStream_t stream) {
  if (x_is_u8) return vbf_down_launch<NB, unsigned char, false>(what, q, grid, stream);
  return vec ? vbf_down_launch<NB, float, true>(what, q, grid, stream) : vbf_down_launch<NB, float, false>(what, q, grid, stream);
}

extern "C" int oniris_vae_wide_conv_a_bf16(const float* S, const uint16_t* w, const float* bias, float* out, int B, int T, int H, int W,
                                           int C, int g, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(S && w && bias && out && (const float*)out != S, "vae_wide_conv_a_bf16: null pointer or out aliases S");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && vae_wide_c_ok(C) && g >= 1 && g <= 8 && T % g == 0,
                   "vae_wide_conv_a_bf16: bad sizes (B %d T %d H %d W %d C %d g %d)", B, T, H, W, C, g);
  ONIRIS_CHECK_ARG((long long)B * (g + T) <= 0x7fffffffLL, "vae_wide_conv_a_bf16: %lld planes", (long long)B * (g + T));
  VaeWideBf16Params q{};
  VaeWideParams& p = q.p;
  q.w = w;
  p.x = S; p.bias = bias; p.out = out;
  p.B = B; p.T = T; p.H = H; p.W = W; p.Cin = C; p.Cout = C; p.nsub = g; p.g = g;
  return vbf_dispatch<VW_CONV_A>("vae_wide_conv_a_bf16", q, (long long)B * (T / g), (hipStream_t)stream);
}

extern "C" int oniris_vae_wide_conv_b_bf16(const float* u, const float* res, const uint16_t* w, const float* bias, float* out, int B,
                                           int T, int H, int W, int C, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(u && res && w && bias && out && (const float*)out != u, "vae_wide_conv_b_bf16: null pointer or out aliases u");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && vae_wide_c_ok(C), "vae_wide_conv_b_bf16: bad sizes (B %d T %d H %d W %d C %d)", B,
                   T, H, W, C);
  VaeWideBf16Params q{};
  VaeWideParams& p = q.p;
  q.w = w; q.res = res;
  p.x = u; p.bias = bias; p.out = out;
  p.B = B; p.T = T; p.H = H; p.W = W; p.Cin = C; p.Cout = C; p.nsub = 1; p.g = 1;
  return vbf_dispatch<VBF_CONV_B>("vae_wide_conv_b_bf16", q, (long long)B * T, (hipStream_t)stream);
}

extern "C" int oniris_vae_wide_up_bf16(const float* x, const uint16_t* w, const float* bias, float* out, int B, int T, int H, int W,
                                       int C, int tcomp, int scomp, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && w && bias && out && (const float*)out != x, "vae_wide_up_bf16: null pointer or out aliases x");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && vae_wide_c_ok(C) && tcomp >= 1 && tcomp <= 2 && scomp >= 1 && scomp <= 2,
                   "vae_wide_up_bf16: bad sizes (B %d T %d H %d W %d C %d tc %d sc %d)", B, T, H, W, C, tcomp, scomp);
  VaeWideBf16Params q{};
  VaeWideParams& p = q.p;
  q.w = w;
  p.x = x; p.bias = bias; p.out = out;
  p.B = B; p.T = T; p.H = H; p.W = W; p.Cin = C; p.Cout = C; p.nsub = tcomp * scomp * scomp; p.g = 1; p.tc = tcomp; p.sc = scomp;
  return vbf_dispatch<VW_UP>("vae_wide_up_bf16", q, (long long)B * T, (hipStream_t)stream);
}

extern "C" int oniris_vae_wide_out_bf16(const float* x, const uint16_t* w, const float* bias, int B, int T, int H, int W, int Cin,
                                        int Cout, int split, const float* logvar_mult, float* out, float* out2, int64_t sb, int64_t st,
                                        int64_t sh, int64_t sw, int64_t sc, uint8_t* frames, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && w && bias && (out || frames), "vae_wide_out_bf16: null pointer");
  ONIRIS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && vae_wide_c_ok(Cin) && vae_wide_c_ok(Cout) && split >= 0 && split < Cout,
                   "vae_wide_out_bf16: bad sizes (B %d T %d H %d W %d Cin %d Cout %d split %d)", B, T, H, W, Cin, Cout, split);
  ONIRIS_CHECK_ARG(split == 0 || (logvar_mult && (out2 || !out)), "vae_wide_out_bf16: the split needs logvar_mult and out2");
  ONIRIS_CHECK_ARG(!frames || split > 0, "vae_wide_out_bf16: frames need the mean / logvar split");
  VaeWideBf16Params q{};
  VaeWideParams& p = q.p;
  q.w = w;
  p.x = x; p.bias = bias; p.out = out; p.out2 = out2; p.frames = (unsigned char*)frames; p.lvm = logvar_mult;
  p.B = B; p.T = T; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.nsub = 1; p.g = 1; p.split = split;
  p.sb = sb; p.st = st; p.sh = sh; p.sw = sw; p.scs = sc;
  return vbf_dispatch<VW_OUT>("vae_wide_out_bf16", q, (long long)B * T, (hipStream_t)stream);
}

extern "C" int oniris_vae_wide_down_bf16(const void* x, int x_is_u8, int64_t sb, int64_t st, int64_t sh, int64_t sw, int64_t sc, int B,
                                         int To, int Ho, int Wo, int Cin, int tcomp, int scomp, int normalize, const uint16_t* w,
                                         const float* bias, int Cout, float* out, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(x && w && bias && out && (const void*)out != x, "vae_wide_down_bf16: null pointer or out aliases x");
  ONIRIS_CHECK_ARG(B > 0 && To > 0 && Ho > 0 && Wo > 0 && vae_wide_c_ok(Cin) && vae_wide_c_ok(Cout) && tcomp >= 1 && tcomp <= 2 &&
                       scomp >= 1 && scomp <= 2,
                   "vae_wide_down_bf16: bad sizes (B %d T %d H %d W %d Cin %d tc %d sc %d Cout %d)", B, To, Ho, Wo, Cin, tcomp, scomp,
                   Cout);
  ONIRIS_CHECK_ARG(vbf_aligned(w, 4), "vae_wide_down_bf16: w must be 4-byte aligned");
  VaeWideDownBf16Params q{};
  VaeWideDownParams& p = q.p;
  q.w = w;
  p.x = x; p.bias = bias; p.out = out;
  p.sb = sb; p.st = st; p.sh = sh; p.sw = sw; p.sc = sc;
  p.B = B; p.To = To; p.Ho = Ho; p.Wo = Wo; p.Cin = Cin; p.Cout = Cout; p.tc = tcomp; p.scm = scomp; p.normalize = normalize;
  p.CinP = roundup(Cin, VBF_KSTEP);
  p.CP = roundup(Cout, 32);
  p.tiles_x = cdiv(Wo, DISC_TILE); p.tiles_y = cdiv(Ho, DISC_TILE);
  const int nb = vae_wide_nb(p.CP);
  p.nblk = p.CP / (32 * nb);
  const long long wgs = (long long)B * To * p.tiles_x * p.tiles_y;
  ONIRIS_CHECK_ARG(wgs <= 0x7fffffffLL && p.nblk <= 65535, "vae_wide_down_bf16: %lld tiles", wgs);
  const bool vec = !x_is_u8 && !normalize && sc == 1 && Cin % 8 == 0 && sb % 4 == 0 && st % 4 == 0 && sh % 4 == 0 && sw % 4 == 0 &&
                   vbf_aligned(x, 16);
  const dim3 grid((unsigned)wgs, p.nblk);
  return nb == 2 ? vbf_down_pick<2>("vae_wide_down_bf16", q, x_is_u8, vec, grid, (hipStream_t)stream)
                 : vbf_down_pick<1>("vae_wide_down_bf16", q, x_is_u8, vec, grid, (hipStream_t)stream);
}
