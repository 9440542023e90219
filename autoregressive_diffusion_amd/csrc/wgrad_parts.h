// The decisions every bf16 weight-gradient kernel (conv_wgrad.hip, conv_wgrad_glds.h, conv_wgrad_stream.h, wgrad1x1_glds.h) has
// to agree on, written once: the launch descriptor of a grouped launch and its group select, the transposing LDS read that makes
// an MFMA fragment and the lane roles it implies, the bf16 rounding of the per-frame coefficient folded into dy, the two tile
// loops (flat (k-step, tap) order | halo-row order) with their scheduling pattern, the meeting in LDS of the waves that hold
// partial sums of one 32x32 tile, the slab layout weight_bwd_kernel reads, and the report of the slab count.  Everything is
// __forceinline__; a loop takes the kernel's own fragment addressing as functors: a kernel compiles to what it was with its
// own copy (profiles/wgrad_shared_parts.txt).
#pragma once
#include "lds_dma.h"
#include "../../include/oniris.h"

// Up to three sub-problems of identical geometry (H, W, channels, taps) share one launch: the own-frame weight and the
// two context taps of a gated conv.  Workgroup columns [gstart[g], gstart[g+1]) belong to group g; every column
// writes ONE slab, so one launch writes as many slabs as three separate ones used to write each.
#define WGRAD_MAXG 3
struct WgradDev {
  OnirisWgradArgs a[WGRAD_MAXG];
  int ntiles[WGRAD_MAXG], ntt[WGRAD_MAXG], gstart[WGRAD_MAXG + 1];
  int ntx, nty, ncib;
};

#ifdef __HIPCC__
// ---- the group of this workgroup column, its place among the group's columns (column bx of gxg walks position tiles bx,
// bx + gxg, ... of the group's ntiles) and the (32 CT co) x (32 IT ci) channel block of blockIdx.y.  conv_wgrad_glds_kernel
// takes it from here; conv_wgrad_kernel, which reads fields of its group inside the tile loop, keeps the same lines in its
// body (through the call hipcc re-derives the group's address at every such read: +1.5 % on the 1x1 form).
struct WgradGroup {
  int gsel, bx, gxg, ntiles, ntt;
  int co0, ci0;
};
template <int CT, int IT>
__device__ __forceinline__ WgradGroup wgrad_group(const WgradDev& d) {
  WgradGroup g;
  g.gsel = 0;
  if ((int)blockIdx.x >= d.gstart[1]) g.gsel = 1;
  if ((int)blockIdx.x >= d.gstart[2]) g.gsel = 2;
  g.bx = blockIdx.x - d.gstart[g.gsel];
  g.gxg = d.gstart[g.gsel + 1] - d.gstart[g.gsel];
  g.ntiles = d.ntiles[g.gsel];
  g.ntt = d.ntt[g.gsel];
  const int cib = blockIdx.y % d.ncib, cob = blockIdx.y / d.ncib;
  g.co0 = cob * 32 * CT;
  g.ci0 = cib * 32 * IT;
  return g;
}

// ---- fragments.  Both operands are staged row-major ([position][channel]) and the reduction runs over positions: the
// k-contiguous MFMA fragment comes from the gfx950 transposing read ds_read_b64_tr_b16 (4 rows x 16 columns per 16-lane group).
// two transposing reads (rows r..r+3 at base0, r+4..r+7 at base1) -> 8 k-contiguous bf16 for this lane's channel
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* base0, const unsigned char* base1) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)base0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)base1);
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  s16x8 v;
  v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
  v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
  return __builtin_bit_cast(bf16x8, v);
}
// lane roles of that read inside a 16-position k-step x 32-channel tile: the lane's first row is 8 hh + q (the second read
// takes the row 4 below) and its four channels start at byte cslot of the tile's 64-byte row
struct WgradLane {
  int hh, q, cslot;
};
__device__ __forceinline__ WgradLane wgrad_lane(int lane) {
  return {lane >> 5, (lane & 15) >> 2, (lane & 3) * 8 + 32 * ((lane >> 4) & 1)};
}
// the per-frame coefficient folded into a dy fragment: one bf16 rounding per value, like a dy2 tensor written to memory
__device__ __forceinline__ bf16x8 wgrad_fold(bf16x8 v, float sc) {
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = f2bf(bf2f(v[k]) * sc);
  return v;
}

// ---- FLAT tile loop: k = 16 positions per step; the NK x TAPS (k-step, tap) pairs form one sequence whose fragment reads
// (ld_a(ksi): dy of k-step ksi, ld_b(ksi, tap): x) run LA MFMAs ahead of their use -- rings of four, the lookahead never laps
// a live fragment -- in an order pinned with sched_group_barrier.
template <int TAPS, int NK, typename LdA, typename LdB>
__device__ __forceinline__ void wgrad_flat_loop(f32x16 (&acc)[TAPS], LdA ld_a, LdB ld_b) {
  constexpr int NSTEP = NK * TAPS;
  constexpr int LA = (NSTEP > 3) ? 3 : 1;               // (a kernel with one wave per SIMD has to cover the LDS latency by itself)
  constexpr int NA0 = (LA + TAPS - 1) / TAPS;
  bf16x8 af[4], bfm[4];
#pragma unroll
  for (int j = 0; j < LA; ++j) {
    if (j % TAPS == 0) af[(j / TAPS) & 3] = ld_a(j / TAPS);
    bfm[j] = ld_b(j / TAPS, j % TAPS);
  }
  __builtin_amdgcn_sched_group_barrier(0x100, 2 * NA0 + 2 * LA, 0);
#pragma unroll
  for (int st = 0; st < NSTEP; ++st) {
    const int ksi = st / TAPS, tap = st % TAPS;
    const int nx = st + LA;
    if (nx < NSTEP) {
      if (nx % TAPS == 0) af[(nx / TAPS) & 3] = ld_a(nx / TAPS);
      bfm[nx & 3] = ld_b(nx / TAPS, nx % TAPS);
    }
    acc[tap] = mfma32(af[ksi & 3], bfm[st & 3], acc[tap]);
    if (nx < NSTEP) {
      if (nx % TAPS == 0) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
      else __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
  }
}

// ---- HALO-ROW ORDER (a wave that owns every k-step of its 32x32 tile, 3x3 taps).  The x fragment of (k-step ks, tap (ky, kx))
// depends on u = ks + ky (PW 16: halo row u) resp. u = 2 ks + ky (PW 8: halo rows u, u + 1) and kx only: walking (u, kx) instead
// of (ks, tap) reads each distinct fragment ONCE (ld_bu(u, kx)) and feeds it to up to three MFMAs -- at NK = 8 (4) k-steps 76
// (70) transposing LDS reads per tile and wave instead of 160 (88), in a loop whose two waves per SIMD issue 2.2 LDS reads per
// MFMA against ~1 the LDS pipe can serve.  Per tap the k-steps are still added in ascending order: the partial sums are
// bit-identical to the flat loop's.
template <int PW, int NK, typename LdA, typename LdBu>
__device__ __forceinline__ void wgrad_halo_row_loop(f32x16 (&acc)[9], LdA ld_a, LdBu ld_bu) {
  static_assert(PW == 16 || PW == 8, "tile widths");
  constexpr int LA = 3, NU = (PW == 16) ? NK + 2 : 2 * NK + 1, NB = NU * 3, AW = (PW == 16) ? 4 : 2;
  bf16x8 aw[AW], bfm[4];
  aw[0] = ld_a(0);
#pragma unroll
  for (int j = 0; j < LA; ++j) bfm[j] = ld_bu(j / 3, j % 3);
  __builtin_amdgcn_sched_group_barrier(0x100, 2 + 2 * LA, 0);
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int u = j / 3, kx = j % 3;
    int nrd = 0, nmf = 0;
    if (j + LA < NB) { bfm[(j + LA) & 3] = ld_bu((j + LA) / 3, (j + LA) % 3); nrd += 2; }
    // the dy fragment of k-step ks is first used at u = ks (PW 16) / u = 2 ks (PW 8): requested one u earlier, into the slot
    // of the k-step whose last use (ky = 2) lies behind
    const int ksn = (PW == 16) ? u + 1 : (u + 1) / 2;
    if (kx == 0 && ksn < NK && ((PW == 16) || (u & 1))) { aw[ksn % AW] = ld_a(ksn); nrd += 2; }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int num = u - ky, ks = (PW == 16) ? num : num / 2;
      if (num >= 0 && ks < NK && ((PW == 16) || (num & 1) == 0)) {
        acc[ky * 3 + kx] = mfma32(aw[ks % AW], bfm[j & 3], acc[ky * 3 + kx]);
        ++nmf;
      }
    }
    if (nrd == 2) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);          // (the builtin takes literals)
    else if (nrd == 4) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
    if (nmf == 1) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    else if (nmf == 2) __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    else __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
  }
}

// ---- the waves that hold partial sums of one 32x32 tile meet in LDS: red = [slot][16][64] floats (4 KB per slot, in the
// staging LDS, which is free by then).  The caller puts a barrier in front of the puts and one between puts and adds.
// my 16 registers of one tap into slot s
__device__ __forceinline__ void wgrad_red_put(float* red, int s, int lane, const f32x16& v) {
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) red[(s * 16 + rr) * 64 + lane] = v[rr];
}
// slots [first, first + cnt) added to my 16 registers, in ascending order
__device__ __forceinline__ void wgrad_red_add(const float* red, int first, int cnt, int lane, f32x16& v) {
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    float s = v[rr];
#pragma unroll
    for (int w = 0; w < cnt; ++w) s += red[((first + w) * 16 + rr) * 64 + lane];
    v[rr] = s;
  }
}
// NPART waves per tile (part 0 keeps the sum, parts 1.. are added to it in ascending order), NTILE tiles per workgroup, tap by
// tap; true for the wave that goes on to write the slab
template <int TAPS, int NPART, int NTILE>
__device__ __forceinline__ bool wgrad_meet(float* red, f32x16 (&acc)[TAPS], int part, int tile, int lane) {
  if constexpr (NPART > 1) {
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) {
      __syncthreads();
      if (part > 0) wgrad_red_put(red, tile * (NPART - 1) + part - 1, lane, acc[tap]);
      __syncthreads();
      if (part == 0) wgrad_red_add(red, tile * (NPART - 1), NPART - 1, lane, acc[tap]);
    }
  }
  return part == 0;
}

// ---- split-K slabs: workgroup column s of a launch writes ITS OWN slab s of the weight with plain stores, bf16
// [slab][CoutP co][taps_total][CinP ci] -- a weight row (all taps of one co) is contiguous -- and weight_bwd_kernel
// (weights.hip) sums the slabs.
__device__ __forceinline__ bf16* wgrad_slab(void* dwp, int s, int taps_total, int CoutP, int CinP) {
  return (bf16*)dwp + (size_t)s * taps_total * CoutP * CinP;
}
// one 32x32 MFMA tile of tap `tap` (of the weight's taps_total): rows co_t + mfma_row, the lane's column cj
__device__ __forceinline__ void wgrad_store_tile(bf16* slab, int tap, int taps_total, int CoutP, int CinP, int co_t, int cj,
                                                 int lane, const f32x16& v) {
  bf16* base = slab + (size_t)tap * CinP;
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int co = co_t + mfma_row(rr, lane);
    if (co < CoutP && cj < CinP) base[(size_t)co * taps_total * CinP + cj] = f2bf(v[rr]);
  }
}
// the number of slabs a launch wrote for a weight (OnirisWgradArgs.nsplit_out), by the first thread of column `col` (by reference:
// only that thread reads the pointer)
__device__ __forceinline__ void wgrad_report_nsplit(int32_t* const& nsplit_out, int col, int nsplit) {
  if (col == 0 && blockIdx.y == 0 && threadIdx.x == 0 && nsplit_out) *nsplit_out = nsplit;
}
#endif
