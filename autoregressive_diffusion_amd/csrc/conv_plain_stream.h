// Plain 3x3 convolution, 32 -> <= 32 channels (the 64x64-pixel level of the UNets in the 2-D training steps -- just_2d,
// edm2/conv.py:60 -- and the data gradients of those layers): STREAMING variant of conv_glds_kernel<NT=1, CTX=false>.
//
// At 32 channels a 16x16-pixel tile of the tile kernel is ONE phase (one 32-channel chunk, no context phases): 42 KB of
// LDS-DMA (both frames' halos + the weight slab, re-copied for every tile) in front of 36 MFMAs per wave and an epilogue
// that stops all eight waves -- 0.44 of its HBM roofline.  The level is HBM-bound by a factor of three (0.5-0.8 GB per
// launch against 31 us of MFMA work at B = 8), so what matters is bytes in flight and that nothing waits for anything else.
// Here (the forward half of conv_stream.h without its context ring; what the two have in common is in conv_parts.h):
//   * a workgroup (4 waves, an 8x16-pixel tile, TWO per CU: they share no barrier and drift apart) owns one spatial tile
//     and WALKS the frames of a segment; per frame it copies ONE halo image (10 x 18 pixels, 11.25 KB) into a four-slot
//     ring, three frames ahead (counted vmcnt: the stores of the previous epilogues drain under the next frames);
//   * the weights (9 taps x 32 x 32) live in REGISTERS for the whole walk, 18 fragments per wave; wave w computes pixel rows
//     2w, 2w + 1 of the tile: 18 MFMAs per frame in two independent chains, one LDS fragment read per MFMA, no exchange
//     between the waves;
//   * epilogues none | emb-scale + SiLU | mp_sum + clip with the clip report (the arithmetic: conv_parts.h), lane =
//     position, bf16 results transposed through the wave's own LDS tile, 16-byte stores (non-temporal on big tensors).
// Same operand rounding (bf16 operands, fp32 accumulation); the summation order over (tap, k) is the tile kernel's with the
// two k-steps of a tap in separate chains, joined at the end.
#pragma once
#include "conv_kernels.h"
#include "lds_dma.h"

struct ConvPlainStreamDev {
  OnirisConvArgs a;
  int ntx, nty, nseg, seglen, nfr;     // nfr = B * S * T frames
  int nt;                              // non-temporal output stores (see conv_stream.h)
};

__global__ __launch_bounds__(256, 2) void conv_plain_stream_kernel(const ConvPlainStreamDev d) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int TAPS = 9, KS = 2, NST = TAPS * KS, HW_ = 18, HALO = 10 * HW_, HBUF = 12288, NRING = 4, DEPTH = 3;
  constexpr int STGB = 32 * CONV_STREAM_EROW;
  constexpr int STG = NRING * HBUF, ESC = STG + 4 * STGB, LDS_BYTES = ESC + NRING * 128;     // emb-scale rows [ring slot][32] fp32
  static_assert(HALO * 64 <= HBUF && 2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");
  __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BYTES];

  const OnirisConvArgs& a = d.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int uw = __builtin_amdgcn_readfirstlane(wave);
  const int H = a.H, W = a.W, HWp = H * W, Cout = a.Cout;
  constexpr int Cin = 32;
  const int frame_elems = HWp * Cin;

  // ---- this workgroup's (tile, segment); workgroup ids go round-robin over the XCDs: XCD k takes a contiguous range of units
  int u = conv_xcd_unit();
  const int x0 = (u % d.ntx) * 16; u /= d.ntx;
  const int y0 = (u % d.nty) * 8;
  const int seg = u / d.nty;
  const int n_lo = seg * d.seglen, n_hi = min(d.nfr, n_lo + d.seglen), nfr = n_hi - n_lo;
  if (nfr <= 0) return;

  // ---- lane -> position inside the wave's 32-position tile (2 pixel rows x 16)
  const int pr = conv_lane_pos<16>(r);
  int xaddr[TAPS];
#pragma unroll
  for (int tap = 0; tap < TAPS; ++tap) {
    const int R = (2 * uw + (pr >> 4) + tap / 3) * HW_ + (pr & 15) + tap % 3;
    xaddr[tap] = R * 64 + ((h ^ ((R >> 2) & 3)) << 4);                   // k-step 1: ^ 32
  }

  // ---- DMA descriptors: 720 pieces of 16 B per halo image, three per thread
  constexpr int OOB = CONV_STREAM_OOB;
  int hv[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int e = i * 256 + tid, row = e >> 2, gp = (e & 3) ^ ((row >> 2) & 3);
    const int y = y0 + row / HW_ - 1, x = x0 + row % HW_ - 1;
    hv[i] = (e < HALO * 4 && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? ((y * W + x) * Cin + gp * 8) * 2 : OOB;
  }
  const i32x4 rs_x = make_rsrc(a.x, d.nfr * frame_elems * 2);
  const unsigned lds0 = (unsigned)(size_t)(lds_void_t*)smem, wdst = lds0 + wave * 1024;
  const bool emb = a.epi == ONIRIS_EPI_EMB_SILU, mps = a.epi == ONIRIS_EPI_MPSUM;
  const int epitch = a.escale_pitch ? a.escale_pitch : Cout;
  const i32x4 rs_e = make_rsrc(a.escale ? a.escale : (const void*)oniris_fill_rows, emb ? (int)(((size_t)d.nfr - 1) * epitch + Cout) * 4 : 0);
  const int evoff = (lane < 8 && lane * 4 < Cout) ? lane * 16 : OOB;    // piece `lane` of the frame's row
  auto issue = [&](int f) __attribute__((always_inline)) {              // halo of frame f (+ its emb-scale row: wave 0)
    const int so = f * frame_elems * 2;
    const unsigned dst = (f & (NRING - 1)) * HBUF + wdst;
    dma16(rs_x, hv[0], so, dst);
    dma16(rs_x, hv[1], so, dst + 4096);
    if (512 + tid < HALO * 4) dma16(rs_x, hv[2], so, dst + 8192);
    if (emb && uw == 0 && lane < 8) dma16(rs_e, evoff, (f * epitch) * 4, lds0 + ESC + (f & (NRING - 1)) * 128);
  };
  // instruction counts of this wave (wave-uniform): copies per frame, residual loads, stores per epilogue
  const int n_dma = 3 + ((emb && uw == 0) ? 1 : 0);                      // (the third halo piece ends inside wave 3: 720 - 512 = 208 lanes)
  const int n_res = mps ? 4 : 0;
  const int n_st = 2 * (mps ? ((a.out2 ? 1 : 0) + 1) : emb ? 2 : 1);

  // ---- weights -> registers (once): lane (r = co row, h = 8-channel group of the k-step)
  bf16x8 wreg[NST];
  conv_stream_weights(wreg, (const bf16*)a.w_own, a, r, h);

  // ---- epilogue inputs (see conv_stream.h: nothing in the frame loop is an ordinary vector load)
  const int ppy = 2 * uw + (pr >> 4), ppx = pr & 15;                     // pixel of this lane's output position inside the 8x16 tile
  const int pix = (y0 + ppy) * W + x0 + ppx;
  ConvStreamRes res;
  res.init(mps ? a.res : (const void*)oniris_fill_rows, mps ? d.nfr * HWp * Cout * 2 : 0, pix, Cout, h);
  constexpr int VM_SAT = 40;                                             // where the counted waits saturate

  // ---- prologue copies: the first DEPTH frames of the segment
#pragma unroll 1
  for (int i = 0; i < DEPTH && i < nfr; ++i) issue(n_lo + i);
  unsigned char* const ep = smem + STG + wave * STGB;                    // this wave's staging tile

#pragma unroll 1
  for (int i = 0; i < nfr; ++i) {
    const int f = n_lo + i;
    // this wave's copies of frame f have landed.  Younger instructions of this wave that may still be in flight: the copies of
    // the frames issued after f's (up to DEPTH - 1 of them, each issued in a step behind that step's residual loads and in
    // front of its stores) and the stores / residual loads of the steps in between
    {
      const int ahead = min(DEPTH - 1, nfr - 1 - i);                     // frames f+1 .. f+ahead are requested
      // steps i-DEPTH+1 .. i-1 issued: [res][dma (if any)][stores]; the copies of frame f+j went out in step i+j-DEPTH (or the prologue)
      int younger = 0;
      for (int j = 1; j <= ahead; ++j) younger += n_dma;
      const int steps_behind = min(i, DEPTH - 1);                         // full steps issued after frame f's copies ... at most
      younger += steps_behind * (n_res + n_st);
      if (i >= DEPTH) younger += n_st;                                    // the stores of step i-DEPTH, issued right after f's copies
      conv_wait_vm<VM_SAT>(younger);
    }
    __syncthreads();                       // ... everybody's have; and everybody is done with frame f - 1 (its ring slot is free)
    typedef const __attribute__((address_space(4))) float cfloat_t;
    const float cown = a.coef_own ? ((cfloat_t*)(size_t)a.coef_own)[f] : 1.f;
    if (mps) res.load((f * HWp * Cout) * 2);     // (in front of the copies: waited for by count, conv_parts.h)
    const bool has_next = i + DEPTH < nfr;
    if (has_next) issue(f + DEPTH);

    f32x16 acc0, acc1;
#pragma unroll
    for (int k = 0; k < 16; ++k) { acc0[k] = 0.f; acc1[k] = 0.f; }
    {
      const unsigned char* bA = smem + (f & (NRING - 1)) * HBUF;
      bf16x8 xf[2];
      xf[0] = *(const bf16x8*)(bA + xaddr[0]);
#pragma unroll
      for (int st = 0; st < NST; ++st) {
        if (st + 1 < NST) {
          const int tap = (st + 1) / KS, ks = (st + 1) % KS;
          xf[(st + 1) & 1] = *(const bf16x8*)(bA + (xaddr[tap] ^ (ks * 32)));
        }
        if (st & 1) acc1 = mfma32(wreg[st], xf[st & 1], acc1);
        else acc0 = mfma32(wreg[st], xf[st & 1], acc0);
        if (st + 1 < NST) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      }
    }
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = cown * (acc0[k] + acc1[k]);

    // ---- epilogue (lane = position; bf16 results transposed through the wave's LDS tile)
    const size_t blk = (size_t)f * HWp;
    ConvStreamOut out;
    out.ep = ep; out.lane = lane; out.pr = pr; out.h = h;
    out.y = y0 + 2 * uw; out.x = x0;
    out.W = W; out.Cout = Cout; out.nontemporal = d.nt != 0;
    if (mps) {
      conv_stream_mpsum<VM_SAT>(a, res, out, v, blk, has_next ? n_dma : 0, [] {});
      continue;
    }
    out.put(v);
    out.flush((bf16*)a.out, blk);
    if (emb) {
      conv_emb_silu16(v, smem + ESC + (f & (NRING - 1)) * 128, 0, h);
      out.put(v);
      out.flush((bf16*)a.out2, blk);
    }
  }
#endif
}

// Shapes the plain streaming kernel takes: S == 1, no context path, 9 taps, exactly 32 input channels, at most 32 output
// channels, images of 8-row x 16-column tiles, the epilogues of the 3x3 layers.
static inline bool conv_plain_stream_ok(const OnirisConvArgs& a) {
  if (!(a.S == 1 && !a.ctx && a.taps == 9 && a.Cin == 32 && a.CinP == 64 && a.CoutP == 32 && a.W % 16 == 0 && a.H % 8 == 0)) return false;
  if (a.ctx_out || a.x2 || a.coef_ctx || a.ctx_prod_mode != 0) return false;
  if (!(a.epi == ONIRIS_EPI_NONE || a.epi == ONIRIS_EPI_EMB_SILU || a.epi == ONIRIS_EPI_MPSUM)) return false;
  if (a.escale_pitch != 0 && a.escale_pitch % 4 != 0) return false;
  const long long nfr = (long long)a.B * a.T;
  if (nfr * a.H * a.W * 32 * 2 >= (1LL << 31) || nfr * (a.escale_pitch ? a.escale_pitch : a.Cout) * 4 >= (1LL << 31)) return false;
  return nfr * (a.H / 8) * (a.W / 16) >= 512;          // (small launches: the tile kernel's single wave of workgroups is as good)
}

static int launch_conv_plain_stream(const OnirisConvArgs& a, hipStream_t stream) {
  ConvPlainStreamDev d;
  d.a = a;
  d.ntx = a.W / 16; d.nty = a.H / 8;
  d.nfr = a.B * a.T;
  const int tiles = d.ntx * d.nty;
  int nseg = 512 / tiles;                  // two workgroups per CU
  if (nseg > d.nfr / 4) nseg = d.nfr / 4;  // (a segment pays its pipeline fill: three frames)
  if (nseg < 1) nseg = 1;
  d.seglen = cdiv(d.nfr, nseg);
  d.nseg = cdiv(d.nfr, d.seglen);
  d.nt = (long long)d.nfr * a.H * a.W * a.Cout * 2 >= oniris_ew_nt_bytes();
  oniris_launch_tagged(d.nt ? "nt-stores" : nullptr, conv_plain_stream_kernel, dim3(tiles * d.nseg), dim3(256), stream, d);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}
