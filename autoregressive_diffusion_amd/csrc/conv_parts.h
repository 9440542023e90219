// The decisions every forward / dgrad conv kernel family has to agree on, written once: the lane -> position map of the
// 3x3 kernels, the XCD-contiguous work distribution, the epilogue arithmetic (mp_sum + clip, emb-scale + SiLU), the store of
// a lane's 16 results into its wave's transpose tile, and what the two streaming kernels (conv_stream.h,
// conv_plain_stream.h) have in common.  Everything is __forceinline__: a kernel compiles to what it was with its own copy.
#pragma once
#include "lds_dma.h"
#include "../../include/oniris.h"

#ifdef __HIPCC__
// ---- lane -> position inside a wave's 32-position tile, r = lane & 31.  PW = 16: the 32 positions (2 patch rows x 16 px)
// are dealt to the lanes so that each 16-lane group of a ds_read_b128 ({0-3,12-15,20-27} / {4-11,16-19,28-31}) reads 16
// CONSECUTIVE halo rows: with 80-byte rows, or with 64-byte rows swizzled by row bits 2..3, that is conflict-free (the natural
// order is 2-way on every read).  PW = 8 (4 patch rows x 8 px, 12-entry halo rows): a read group takes patch rows (0,2)
// resp. (1,3), i.e. halo rows 24 = 8 (mod 16) apart.
template <int PW>
__device__ __forceinline__ int conv_lane_pos(int r) {
  static_assert(PW == 16 || PW == 8, "tile widths of the 3x3 kernels");
  const bool ga = (r < 4) || (r >= 12 && r < 16) || (r >= 20 && r < 28);
  const int k = ga ? ((r < 4) ? r : (r < 16) ? r - 8 : r - 12) : ((r < 12) ? r - 4 : (r < 20) ? r - 8 : r - 16);
  if constexpr (PW == 16) return (ga ? 0 : 16) + k;
  else return ((k >> 3) * 2 + (ga ? 0 : 1)) * 8 + (k & 7);
}

// ---- work distribution.  Workgroup ids go round-robin over the 8 XCDs; XCD k takes the CONTIGUOUS range [lo, hi) of the
// launch's n work items, so items that share input rows (neighbouring tiles, other channel blocks, the frames whose context a
// frame is) run at the same time behind the same L2.
// persistent workgroups: this XCD's range and the number of workgroups (`step`) that walk it together
__device__ __forceinline__ void conv_xcd_range(int n, int& lo, int& hi, int& step) {
  const int nwg = gridDim.x, xcd = blockIdx.x & 7;
  const int q = n >> 3, rr = n & 7;
  lo = (xcd < rr) ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q;
  hi = lo + q + ((xcd < rr) ? 1 : 0);
  step = (nwg - xcd + 7) >> 3;
}
// one item per workgroup (gridDim.x items): the workgroup's item
__device__ __forceinline__ int conv_xcd_unit() {
  int lo, hi, step;
  conv_xcd_range(gridDim.x, lo, hi, step);
  return lo + (blockIdx.x >> 3);
}

// ---- epilogue elements (fp32 in, the caller rounds to bf16)
// mp_silu of z
__device__ __forceinline__ float conv_silu(float z) { return z * sigmoid_fast(z) * (1.f / 0.596f); }
// ONIRIS_EPI_EMB_SILU: the activation sees the bf16-rounded y
__device__ __forceinline__ float conv_emb_silu(float y, float c) { return conv_silu(bf2f(f2bf(y)) * c); }
// p + s with no fma made of it, whatever produced p and s
__device__ __forceinline__ float conv_add_rounded(float p, float s) {
#pragma clang fp contract(off)
  return p + s;
}
// ONIRIS_EPI_MPSUM: ta * res + tb * y, clamped to +-clip where clip > 0.  hit: the clip report (OnirisConvArgs.clip_flag) --
// what the backward's mask tests is the STORED value.  The plain spelling of the sum is open to the compiler's contraction
// (the tile kernels: an fma for some of a lane's values, two rounded products for the others;
// profiles/conv_shared_parts.txt).  TWO_PRODUCTS pins the streaming kernels' form: both products rounded, for every value.
template <bool TWO_PRODUCTS = false>
__device__ __forceinline__ float conv_mpsum(float res, float y, float ta, float tb, float clip, bool& hit) {
  float q = TWO_PRODUCTS ? conv_add_rounded(ta * res, tb * y) : ta * res + tb * y;
  if (clip > 0.f) {
    q = fminf(fmaxf(q, -clip), clip);
    hit |= !(fabsf(bf2f(f2bf(q))) < clip);
  }
  return q;
}
// ... in the kernels that do not report clips (conv_api.hip answers for them)
__device__ __forceinline__ float conv_mpsum(float res, float y, float ta, float tb, float clip) {
  bool unreported = false;
  return conv_mpsum(res, y, ta, tb, clip, unreported);
}
// emb-scale + SiLU of a lane's 16 values; esc: fp32 scales in LDS, c0: the first of the 32 of the lane's channel tile
__device__ __forceinline__ void conv_emb_silu16(float (&v)[16], const unsigned char* esc, int c0, int h) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 ev = *(const float4*)(esc + (c0 + 8 * g + 4 * h) * 4);
    const float cvv[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) v[4 * g + k] = conv_emb_silu(v[4 * g + k], cvv[k]);
  }
}
// a wave raises the launch's clip flag (practically never: OnirisConvArgs.clip_flag); true (wave-uniform) if it did
__device__ __forceinline__ bool conv_report_clip(int* clip_flag, bool hit, int lane) {
  if (clip_flag && __builtin_amdgcn_ballot_w64(hit) != 0ull) {
    if (lane == 0) atomicOr(clip_flag, 1);
    return true;
  }
  return false;
}

// ---- a lane's 16 MFMA results (rows 8 g + 4 h + k of one 32-channel tile) as bf16 into its row of the wave's transpose
// tile; col = first channel of the tile inside the row
__device__ __forceinline__ void conv_stage_row(unsigned char* row, int col, int h, const float (&v)[16]) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    bf16x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = f2bf(v[4 * g + k]);
    *(bf16x4*)(row + (col + 8 * g + 4 * h) * 2) = o;
  }
}

// ---- the streaming pair (32 -> <= 32 channels, a workgroup walks the frames of a segment; conv_stream.h has the reasons)
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
constexpr int CONV_STREAM_OOB = (int)0x80000000;     // a per-lane offset beyond every num_records: the load returns zeros
constexpr int CONV_STREAM_EROW = 80;                 // bytes per row of a wave's staging tile (32 bf16 + 16)

// the 9 x 2 weight fragments of a 32 x 32 slab into registers, once: lane (r = co row, h = 8-channel group of the k-step)
__device__ __forceinline__ void conv_stream_weights(bf16x8 (&wreg)[18], const bf16* wsrc, const OnirisConvArgs& a, int r, int h) {
#pragma unroll
  for (int i = 0; i < 18; ++i) wreg[i] = *(const bf16x8*)(wsrc + ((size_t)(i / 2) * a.CoutP + r) * a.CinP + (i % 2) * 16 + h * 8);
#pragma unroll
  for (int i = 0; i < 18; ++i) asm volatile("" : "+v"(wreg[i]));        // consumed before any LDS-DMA is in flight
}

// s_waitcnt vmcnt(n), n wave-uniform; n >= SAT waits for SAT (waiting for more than asked is always correct)
template <int SAT>
__device__ __forceinline__ void conv_wait_vm(int n) {
  static_assert(SAT <= 40, "cases below");
  switch (n) {      // (a case from SAT on falls through to the default)
#define CONV_VMW(k) case k: if constexpr (k < SAT) { asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break; } [[fallthrough]];
    CONV_VMW(0) CONV_VMW(1) CONV_VMW(2) CONV_VMW(3) CONV_VMW(4) CONV_VMW(5) CONV_VMW(6) CONV_VMW(7) CONV_VMW(8) CONV_VMW(9)
    CONV_VMW(10) CONV_VMW(11) CONV_VMW(12) CONV_VMW(13) CONV_VMW(14) CONV_VMW(15) CONV_VMW(16) CONV_VMW(17) CONV_VMW(18) CONV_VMW(19)
    CONV_VMW(20) CONV_VMW(21) CONV_VMW(22) CONV_VMW(23) CONV_VMW(24) CONV_VMW(25) CONV_VMW(26) CONV_VMW(27) CONV_VMW(28) CONV_VMW(29)
    CONV_VMW(30) CONV_VMW(31) CONV_VMW(32) CONV_VMW(33) CONV_VMW(34) CONV_VMW(35) CONV_VMW(36) CONV_VMW(37) CONV_VMW(38) CONV_VMW(39)
#undef CONV_VMW
    default: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(SAT) : "memory"); break;
  }
}

// The residual of ONIRIS_EPI_MPSUM: four buffer loads per lane and frame through inline asm (hipcc cannot see them, so it
// inserts no wait of its own), issued at the top of a step and waited for by count right before the epilogue uses them.
struct ConvStreamRes {
  i32x4 rs;
  u32x2 q[4];
  int voff[4];
  // base / bytes: the frames this workgroup walks (a 0-byte range when the epilogue is another one); pix: the lane's pixel
  __device__ __forceinline__ void init(const void* base, int bytes, int pix, int Cout, int h) {
    rs = make_rsrc(base, bytes);
#pragma unroll
    for (int g = 0; g < 4; ++g) { q[g][0] = 0u; q[g][1] = 0u; }
#pragma unroll
    for (int g = 0; g < 4; ++g) voff[g] = (8 * g + 4 * h < Cout) ? (pix * Cout + 8 * g + 4 * h) * 2 : CONV_STREAM_OOB;
  }
  __device__ __forceinline__ void load(int frame_off) {          // frame_off: byte offset of the frame, wave-uniform
    const int so = __builtin_amdgcn_readfirstlane(frame_off);
#pragma unroll
    for (int g = 0; g < 4; ++g)
      asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen" : "=v"(q[g]) : "v"(voff[g]), "s"(rs), "s"(so) : "memory");
  }
  __device__ __forceinline__ void arrived() {                    // behind the counted wait: the values are defined from here on
#pragma unroll
    for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(q[g]));
  }
};

// A wave's way out: lane = position `pr` of a tile of 2 pixel rows x 16, bf16 results transposed through the wave's LDS tile
// `ep`, 16-byte stores (non-temporal on big tensors: nothing re-reads them from a cache).
struct ConvStreamOut {
  unsigned char* ep;
  int lane, pr, h;
  int y, x;                                                      // first pixel of the wave's tile
  int W, Cout;
  bool nontemporal;
  __device__ __forceinline__ void put(const float (&v)[16]) const { conv_stage_row(ep + pr * CONV_STREAM_EROW, 0, h, v); }
  __device__ __forceinline__ void flush_row(bf16* dst, size_t fblk, int it) const {      // pixel row `it` of the tile
    const int id = it * 64 + lane, row = id >> 2, part = id & 3;
    const size_t px_ = (size_t)(y + (row >> 4)) * W + x + (row & 15);
    if (part * 8 < Cout) {
      const u32x4 v_ = *(const u32x4*)(ep + row * CONV_STREAM_EROW + part * 16);
      u32x4* o_ = (u32x4*)(dst + (fblk + px_) * Cout + part * 8);
      if (nontemporal) __builtin_nontemporal_store(v_, o_); else *o_ = v_;
    }
  }
  __device__ __forceinline__ void flush(bf16* dst, size_t fblk) const {
    flush_row(dst, fblk, 0);
    flush_row(dst, fblk, 1);
  }
};

// The mp_sum epilogue of a step: v = the lane's 16 conv results, fblk = pixel offset of the frame in the output tensors.
// The residual loads of the step are older than its copies: `younger` instructions may still be in flight.  `before_stores`
// runs between the arithmetic and the stores (conv_stream_kernel: the context product y3).
template <int SAT, typename F>
__device__ __forceinline__ void conv_stream_mpsum(const OnirisConvArgs& a, ConvStreamRes& res, const ConvStreamOut& out,
                                                  const float (&v)[16], size_t fblk, int younger, F before_stores) {
  conv_wait_vm<SAT>(younger);
  res.arrived();
  float o[16];
  bool clip_hit = false;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const bf16x4 rv = __builtin_bit_cast(bf16x4, res.q[g]);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[4 * g + k] = conv_mpsum<true>(bf2f(rv[k]), v[4 * g + k], a.ta, a.tb, a.clip, clip_hit);
  }
  before_stores();
  if (a.out2) { out.put(v); out.flush((bf16*)a.out2, fblk); }
  out.put(o);
  out.flush((bf16*)a.out, fblk);
  if (conv_report_clip(a.clip_flag, clip_hit, out.lane))
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // one more op in the vmcnt stream than the counted waits know
}
#endif
