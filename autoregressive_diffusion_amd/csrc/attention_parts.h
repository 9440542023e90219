// Tile parts shared by the attention kernels of attention.hip (grid kernels), attention_ws.h / attention_bwd_ws.h /
// attention_bwd_dq_ws.h (persistent kernels) and attention_frame.h (frame kernels): the LDS images of a [tokens][64 channels]
// bf16 tile and their swizzles, the fragment reads of those images, the own-row load and the lane-row store, the BlockMask row
// held in a VGPR, the per-thread DMA descriptors of the double-buffered grid kernels and the work-item decode of the persistent
// ones.  Included by attention.hip ahead of the other attention headers.
//
// Nothing here reads threadIdx: every helper takes its lane-derived values as arguments, because the persistent kernels
// re-derive them per work item from a laundered copy of the lane id (see attention_ws.h) and each kernel decides where its
// address registers are computed.  The sched_group_barrier pins and the slot order of the pipelines stay in their kernels.
#pragma once
#include "common.h"
#include "lds_dma.h"

// voffset of an LDS-DMA piece that must read zeros: beyond num_records of every buffer resource
constexpr int OOB = (int)0x80000000;

// ---- LDS images of a tile ------------------------------------------------------------------------------------------
// A tile row is 128 unpadded bytes = eight 16-byte chunks (the DMA image is lane-linear, so there is no room for padding);
// chunk c of row R is stored at chunk c ^ f(R), applied on the SOURCE side of the copy (the lane that writes LDS chunk p of row R
// fetches global chunk p ^ f(R)) and again on the fragment-address side.  Three f, by how the tile is read:
//   row_image   row reads only (ds_read_b128: lane r takes chunk 2 ks + h of row r; an access group is 16 lanes = 16 rows, e.g.
//               rows 0-3, 12-15, 20-27): over the rows of a group f takes all eight values, each for one even and one odd row, and
//               a row step is half of the 64 banks -- the 16 reads cover the banks once, conflict-free;
//   tr_image    transposing reads (ds_read_b64_tr_b16: a 16-lane group takes 4 rows x 64 bytes): rows R and R + 2 of the group
//               would meet in the same banks, f moves bit 1 of the row into chunk bit 2.  Row reads of this image are 4-way
//               conflicted;
//   dual_image  ONE image for both kinds of read of a tile: f = bit1(R) << 2 | bit3(R) << 1 | bit2(R).  Chunk bit 2 still
//               separates rows R / R + 2 for the transposing read, chunk bits 1 and 0 take row bits 3 and 2, so the 16 rows of a
//               row-read access group spread over all eight positions -- both kinds of read are conflict-free (bank model of
//               MI355X_MICROARCH.md, LDS section; the transposing-read swizzle alone left the row reads 4-way conflicted, and
//               with four compute waves on one LDS that was the persistent dK / dV kernel's bound).
__device__ __forceinline__ constexpr int row_image(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ constexpr int tr_image(int row) { return 4 * ((row >> 1) & 1); }
__device__ __forceinline__ constexpr int dual_image(int row) { return (((row >> 1) & 1) << 2) | (((row >> 3) & 1) << 1) | ((row >> 2) & 1); }
enum { IMG_ROW = 0, IMG_TR = 1, IMG_DUAL = 2 };
template <int IMG>
__device__ __forceinline__ constexpr int image_of(int row) { return IMG == IMG_ROW ? row_image(row) : IMG == IMG_TR ? tr_image(row) : dual_image(row); }

// source side: byte offset, inside a [rows][C] bf16 tensor, of what lands in LDS chunk `pp` of tile row `row` (head `head`)
template <int IMG>
__device__ __forceinline__ int image_src(int row, int pp, int C, int head) { return (row * C + head * 64 + (pp ^ image_of<IMG>(row)) * 8) * 2; }

// ---- row fragments: rows r = lane & 31 of a 32-row block, channels ks * 16 + h * 8 + 0..7 (h = lane >> 5) of k-step ks --------
// byte offset of the lane's chunk at k-step 0 (f = the image's swizzle of row r); k-step ks is at base ^ (ks * 32)
__device__ __forceinline__ int row_frag_base(int r, int h, int f) { return r * 128 + ((h ^ f) << 4); }
__device__ __forceinline__ void row_frag(bf16x8 (&f)[4], const unsigned char* tile, int base, int off) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) f[ks] = *(const bf16x8*)(tile + ((base ^ (ks * 32)) + off));
}
// two tiles read side by side, k-step by k-step: the order in which two interleaved MFMA chains (S and dP) consume them, so the
// counted LDS waits in front of the chains stay as fine as the reads (with one tile's reads gathered first hipcc placed eight
// fewer, coarser waits in the pinned loop of attn_bwd_dq_ws_kernel)
__device__ __forceinline__ void row_frag2(bf16x8 (&f0)[4], bf16x8 (&f1)[4], const unsigned char* tile0, int base0, const unsigned char* tile1,
                                          int base1, int off) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    f0[ks] = *(const bf16x8*)(tile0 + ((base0 ^ (ks * 32)) + off));
    f1[ks] = *(const bf16x8*)(tile1 + ((base1 ^ (ks * 32)) + off));
  }
}

// ---- transposed fragments through the gfx950 transposing LDS read -----------------------------------------------------
// tr_read / dual_read(tile, lane roles, tokbase, dt): this lane gets channel dt * 32 + (lane & 31) of the 8 tokens
// {tokbase + 4 hh + 0..3, tokbase + 8 + 4 hh + 0..3} (tokbase a multiple of 16) -- exactly the k order in which an S^T / P
// accumulator (rows = tokens) is consumed as the other MFMA operand.  Lane (grp = lane >> 4, q4, p = lane & 3) of the two reads
// takes row tokbase + 4 hh + q4 (+ 8 for the second), hh = grp >> 1, logical bytes 8 p + 32 (grp & 1) + 64 dt of it.  Bit 1 of
// that row is bit 1 of q4 in both reads, and chunk bit 2 is what it flips in tr_image and dual_image alike: `sw` flips dt.
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
__device__ __forceinline__ bf16x8 tr_pair(const unsigned char* pa, const unsigned char* pb) {
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)pa);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)pb);
  s16x8 v;
  v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
  v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
  return __builtin_bit_cast(bf16x8, v);
}
// transposing image: the second read is the same chunk eight rows on (tr_image ignores row bit 3)
struct TrLane { int base, sw; };
__device__ __forceinline__ TrLane tr_lane(int lane) {
  const int grp = lane >> 4, hh = grp >> 1, q4 = (lane & 15) >> 2, pcol = (lane & 3) * 4 + 16 * (grp & 1);
  return TrLane{(4 * hh + q4) * 128 + pcol * 2, tr_image(q4) >> 2};
}
__device__ __forceinline__ bf16x8 tr_read(const unsigned char* tile, const TrLane& t, int tokbase, int dt) {
  const unsigned char* p0 = tile + t.base + tokbase * 128 + ((dt ^ t.sw) * 64);
  return tr_pair(p0, p0 + 8 * 128);
}
// dual-use image: chunk c = 2 (grp & 1) + (p >> 1) + 4 dt sits at c ^ dual_image(row); its low two bits are hh (row bit 2) and,
// in the second read only, 2 (row bit 3)
struct DualLane { int a, b, sw; };
__device__ __forceinline__ DualLane dual_lane(int lane) {
  const int grp = lane >> 4, hh = grp >> 1, q4 = (lane & 15) >> 2, c0 = 2 * (grp & 1) + ((lane & 3) >> 1);
  // dual_image(4 hh + q4) & 3 = hh, dual_image(4 hh + q4 + 8) & 3 = hh ^ 2, written out: the compiler does not see that row bit 3 is
  // clear in the first read and set in the second
  return DualLane{(4 * hh + q4) * 128 + ((c0 ^ hh) << 4) + 8 * (lane & 1), (4 * hh + q4 + 8) * 128 + ((c0 ^ hh ^ 2) << 4) + 8 * (lane & 1),
                  dual_image(q4) >> 2};
}
__device__ __forceinline__ bf16x8 dual_read(const unsigned char* tile, const DualLane& t, int tokbase, int dt) {
  const int o = tokbase * 128 + ((dt ^ t.sw) * 64);
  return tr_pair(tile + t.a + o, tile + t.b + o);
}

// ---- own rows and lane rows --------------------------------------------------------------------------------------------
// this lane's half of a 64-channel row from global memory as four k-step fragments, or zeros: p = the row's head slot + h * 8
__device__ __forceinline__ void own_row(bf16x8 (&f)[4], const bf16* p, bool in) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    u32x4 v = u32x4{0u, 0u, 0u, 0u};
    if (in) v = *(const u32x4*)(p + ks * 16);
    f[ks] = __builtin_bit_cast(bf16x8, v);
  }
}
// a lane row: the transposed accumulators acc[dt][4 g + k] of a lane (lane = token) are channel lane_row_ch(dt, g, h) + k of
// the token's 64-channel head slot
__device__ __forceinline__ constexpr int lane_row_ch(int dt, int g, int h) { return dt * 32 + 8 * g + 4 * h; }
__device__ __forceinline__ void lane_row_store(bf16* og, const f32x16 (&acc)[2], float scale, int h) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      bf16x4 ov;
#pragma unroll
      for (int k = 0; k < 4; ++k) ov[k] = f2bf(acc[dt][4 * g + k] * scale);
      *(bf16x4*)(og + lane_row_ch(dt, g, h)) = ov;
    }
}
// the same map, fp32 and unscaled (split-KV partials, dK / dV chunk partials)
__device__ __forceinline__ void lane_row_store_f32(float* og, const f32x16 (&acc)[2], int h) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *(float4*)(og + lane_row_ch(dt, g, h)) = make_float4(acc[dt][4 * g], acc[dt][4 * g + 1], acc[dt][4 * g + 2], acc[dt][4 * g + 3]);
}

// ---- grid kernels: one row of the BlockMask table, and the double-buffered tile copies ---------------------------------------
// The row's block list sits in one VGPR (lane i = entry i; rows with more than 64 entries fall back to memory): a scalar load
// per tile put ~1 us of load latency into every iteration.  idx == nullptr: no table, entry j is block j.
struct BlockList {
  const int32_t* idx;      // the row's entries in memory
  int nent, vl, tshift;    // entries, this lane's entry, log2(table block / 128)
  int nsub;                // 64-token tiles of the list
  // first token of 64-token tile `sub` of the list
  __device__ __forceinline__ int start(int sub) const {
    const int j = sub >> 1, jj = j >> tshift;
    int e = j;
    if (idx) e = ((nent <= 64 ? __builtin_amdgcn_readlane(vl, jj) : idx[jj]) << tshift) + (j & ((1 << tshift) - 1));
    return e * 128 + (sub & 1) * 64;
  }
};
// (L = length of the listed sequence: without a table every 128-token block of it is listed)
__device__ __forceinline__ BlockList block_list(const int32_t* num, const int32_t* idx, int cols, int trow, int tshift, int lane, int L) {
  BlockList l;
  l.idx = idx ? idx + (size_t)trow * cols : nullptr;
  l.nent = num ? num[trow] : 0;
  l.vl = (idx && lane < l.nent) ? l.idx[lane] : 0;
  l.tshift = tshift;
  l.nsub = (num ? (num[trow] << tshift) : (L + 127) / 128) * 2;
  asm volatile("" ::"v"(l.vl));                      // consume the ordinary load before any LDS-DMA is in flight
  return l;
}
// DMA descriptors of a thread: NPC 16-byte pieces per tile and tensor, NTS threads per tile; tile row and the source offsets of
// two tensors staged side by side ([IMG0 image | IMG1 image], TB bytes each)
template <int NPC>
struct TilePieces { int row[NPC], vo0[NPC], vo1[NPC]; };
template <int IMG0, int IMG1, int NPC, int NTS>
__device__ __forceinline__ TilePieces<NPC> tile_pieces(int tis, int C, int head) {
  TilePieces<NPC> p;
#pragma unroll
  for (int i = 0; i < NPC; ++i) {
    const int e = i * NTS + tis, row = e >> 3, pp = e & 7;
    p.row[i] = row;
    p.vo0[i] = image_src<IMG0>(row, pp, C, head);
    p.vo1[i] = image_src<IMG1>(row, pp, C, head);
  }
  return p;
}
// request the 64-row tile that starts at token tok0 of both tensors (L tokens each, rows past L read zeros) into dst | dst + TB
template <int NPC, int NTS>
__device__ __forceinline__ void tile_issue(const TilePieces<NPC>& p, const i32x4& rs0, const i32x4& rs1, int tok0, int L, int C, unsigned dst) {
  constexpr int TB = 64 * 128;
  const int left = L - tok0, so = tok0 * C * 2;
#pragma unroll
  for (int i = 0; i < NPC; ++i) {
    const bool ok = p.row[i] < left;
    dma16(rs0, ok ? p.vo0[i] : OOB, so, dst + i * (NTS * 16));
    dma16(rs1, ok ? p.vo1[i] : OOB, so, dst + TB + i * (NTS * 16));
  }
}

// ---- persistent kernels: the work list ----------------------------------------------------------------------------------
// a workgroup's list of work items (oniris_attn_schedule): entry i, or -1 past the end
struct WorkList {
  const int32_t* sched;
  int nslots;
  __device__ __forceinline__ int at(int i) const { return i < nslots ? __builtin_amdgcn_readfirstlane(sched[i]) : -1; }
};
// item = (batch, head) pair << 16 | block index inside the pair
struct WorkItem { int b, head, blk; };
__device__ __forceinline__ WorkItem item_decode(int item, int heads) {
  const int pair = item >> 16, b = pair / heads;
  return WorkItem{b, pair - b * heads, item & 0xffff};
}

// The loader waves' ring loop (counted vmcnt, barrier_j, E1, E2) stays written out in each persistent kernel: as one template over
// the block request it compiled to the same protocol, but with it and the lane set-up lines shared attn_fwd_ws_kernel measured
// 0.9 .. 1.5 % slower in three bench calls and a direct timing, its work item instruction-identical, and not with its own lines back
// (profiles/attn_shared_parts.txt, step 5).
