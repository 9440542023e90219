// VideoAttention / FrameAttention kernels for gfx950 (head dim 64, MFMA 32x32x16 bf16 -> fp32).
//
// Flash-style block-sparse attention that consumes the reference's BlockMask table (128-token kv blocks per
// 128-token q block, bit-exact copy of make_train_mask / make_infer_mask) and applies mask_mod per element on
// partially masked tiles -- the semantics of the compiled FlexAttention kernel.
//
// Forward / dQ: one workgroup = 128 query rows (4 waves x 32 rows), S^T = K.Q^T is computed with the KEY index on
// the MFMA rows and the QUERY on the lanes, so a lane owns one query row: row max / row sum are 32 in-register ops
// plus one cross-half shuffle, and the S^T accumulator is directly the B operand of O^T += V^T.P^T (no LDS round
// trip).  K / V tiles (64 keys) go global -> LDS by LDS-DMA one tile ahead, row-major in unpadded, swizzled 128-byte
// rows; row fragments are 16-byte reads, the transposed operands (V^T, K^T, Q^T, dO^T: MFMA k index = token) come
// from the SAME tiles through the gfx950 transposing read ds_read_b64_tr_b16.  dK/dV: one workgroup = 128 keys,
// lane = key, S = Q.K^T with queries on the rows, P and dS feed dV^T += dO^T.P and dK^T += Q^T.dS from registers.
// The tile images, their fragment reads, the own-row load, the lane-row store, the table row in a VGPR and the tile
// copies are in attention_parts.h, shared with the persistent (attention_*ws.h) and frame (attention_frame.h) kernels.
#include <type_traits>
#include "common.h"
#include "lds_dma.h"
#include "../../include/oniris.h"
#include "attention_parts.h"

#define NEG_BIG (-1.0e30f)
// Softmax without a running maximum: VideoAttention / FrameAttention L2-normalise every 64-vector of q and k to
// norm 8 (attention_modules.py:38) and the xPos factor of an ALLOWED (causal) pair is <= 1 (RoPe.py:60-67), so
// |q.k|/8 <= 8 and the log2-domain score is within +-11.6: exp2(score - SOFTMAX_OFF) cannot overflow, and dropping
// the max / rescale work removes about three quarters of the per-element VALU instructions (the kernel is
// VALU-bound at head dim 64: 256 MFMA FLOP per score element against ~10 VALU instructions with a running max).
#define SOFTMAX_OFF 12.0f
#define SCALE_LOG2 (0.125f * 1.4426950408889634f)

struct AttnDev {
  OnirisAttnArgs a;
  int pshift;     // log2(P)
  int qf_off;     // (Lk - Lq) / P  (frame offset of the queries inside the key sequence, mask_mode 1)
  int tshift;     // log2(table block / 128): the BlockMask BLOCK_SIZE is P when P >= 128
};

// ---- mask_mod on token indices ---------------------------------------------------------------------------------
template <int MODE>
__device__ __forceinline__ bool tok_allowed(int qtok, int ktok, int pshift, int T, int qf_off) {
  if (MODE == 0) return true;
  const int qf = qtok >> pshift, kf = ktok >> pshift;
  if (MODE == 1) return kf <= qf + qf_off;
  // TrainingMask (attention_masking.py:15-24): clean q sees clean kf <= qf; noisy q (f = qf-T) sees clean kf < f
  // and its own noisy frame.
  if (qf < T) return kf <= qf;
  return (kf < T && kf < qf - T) || (kf == qf);
}

// 0 = nothing allowed, 1 = partially masked, 2 = everything allowed, for token ranges [q0,q1] x [k0,k1]
template <int MODE>
__device__ __forceinline__ int classify(int q0, int q1, int k0, int k1, int pshift, int T, int qf_off) {
  if (MODE == 0) return 2;
  const int qa = q0 >> pshift, qb = q1 >> pshift, ka = k0 >> pshift, kb = k1 >> pshift;
  if (MODE == 1) {
    if (kb <= qa + qf_off) return 2;
    if (ka > qb + qf_off) return 0;
    return 1;
  }
  if (qb < T) {                       // clean queries (a 128-token block never straddles the clean|noisy border)
    if (kb <= qa) return 2;
    if (ka > qb) return 0;
    return 1;
  }
  if (kb < T) {                       // noisy queries, clean keys
    if (kb < qa - T) return 2;
    if (ka >= qb - T) return 0;
    return 1;
  }
  if (ka == kb && qa == qb && ka == qa) return 2;
  if (kb < qa || ka > qb) return 0;
  return 1;
}

__device__ __forceinline__ bf16x8 pack8(const f32x16& v, int s2) {
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = f2bf(v[8 * s2 + e]);
  return o;
}

// XCD-aware workgroup order: hardware deals consecutive workgroup ids round-robin to the 8 XCDs (each with its own
// 4 MB L2).  All workgroups of one (batch, head) pair read the same K / V (1 MB each at L = 8192), so a pair is
// pinned to ONE XCD whenever the number of pairs is a multiple of 8: x = position inside the pair's row of the grid,
// bh = pair index.  (Measured: without it K/V stream from the Infinity Cache, ~1 us per tile.)
__device__ __forceinline__ void attn_block_decode(int& x, int& head, int& b) {
  const int nx = gridDim.x, nbh = gridDim.y * gridDim.z;
  const int L = blockIdx.x + nx * (blockIdx.y + gridDim.y * blockIdx.z);
  int bh;
  if ((nbh & 7) == 0) {
    const int xcd = L & 7, k = L >> 3;
    bh = xcd + 8 * (k / nx);
    x = k % nx;
  } else {                                           // (the grid's own coordinates: no division)
    x = blockIdx.x; head = blockIdx.y; b = blockIdx.z;
    return;
  }
  head = bh % gridDim.y;
  b = bh / gridDim.y;
}

// ================================================================================================================
// forward.  K / V tiles (64 keys x 64 channels, 128-byte rows) go global -> LDS by LDS-DMA into two alternating
// buffers: the copy of tile i+1 runs under the MFMA / softmax work of tile i, one barrier per tile, no staging
// registers.  The rows are unpadded (the DMA image is lane-linear), so the 16-byte pieces are XOR-swizzled on the
// source side: K (read row-wise, ds_read_b128, 16 rows per access group) in the row image, V (read through the
// transposing ds_read_b64_tr_b16, 4 rows x 64 bytes) in the transposing image of attention_parts.h.
// KS key streams per workgroup: the 4 waves are 4/KS query waves (32 rows each) x KS streams; stream j walks the key
// tiles j, j+KS, ... of the block's list (own LDS buffers) and the streams' (O, l) partial results meet in LDS at the
// end -- without a running max they simply add.  With a causal table the last query blocks have the longest lists
// and set the launch time; KS = 2 halves that critical path.
template <int MODE, int KS>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(const AttnDev d) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int TB = 64 * 128;                     // bytes of one tile
  constexpr int QW = 4 / KS, NTS = 64 * QW, NPC = 512 / NTS;      // query waves, threads per stream, pieces per thread and tile
  __shared__ __attribute__((aligned(16))) unsigned char smem[KS * 2 * 2 * TB];     // [stream][buffer][K | V]
  const OnirisAttnArgs& a = d.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 31, h = lane >> 5;
  const int qwv = wave % QW, st = wave / QW, tis = tid % NTS;
  // split-KV (decode of one frame against a long KV ring: Lq / 128 query blocks x heads x B workgroups is a handful):
  // kv_splits workgroups share a query block, each walks a contiguous range of its key tiles and leaves an un-normalised
  // partial (O, l) in split_ws; attn_split_reduce_kernel adds them (no running maximum here: partials simply add)
  const int nsp = (MODE == 0 && KS == 1 && a.kv_splits > 1) ? a.kv_splits : 1;
  int bx_, head, b;
  attn_block_decode(bx_, head, b);
  const int nqb = (nsp == 1) ? (int)gridDim.x : (int)gridDim.x / nsp;
  const int sp = (nsp == 1) ? 0 : bx_ % nsp;
  const int qbw = nqb - 1 - ((nsp == 1) ? bx_ : bx_ / nsp);      // heaviest (latest) query blocks first
  const int C = a.C, Lq = a.Lq, Lk = a.Lk;
  const int qw0 = qbw * (32 * QW) + qwv * 32;
  const int qrow = qw0 + r;
  const int qb = (qbw * (32 * QW)) >> 7;           // 128-token block of the mask table

  const bf16* qg = (const bf16*)a.q + (size_t)b * Lq * C + head * 64;
  bf16x8 qf[4];
  own_row(qf, qg + (size_t)qrow * C + h * 8, qrow < Lq);
  f32x16 o[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) { o[0][i] = 0.f; o[1][i] = 0.f; }
  float l2[2] = {0.f, 0.f};                        // this lane's half of the row sum (two chains: packed adds)

  const BlockList kvl = block_list(a.kv_num, a.kv_idx, a.tab_cols, qb >> d.tshift, d.tshift, lane, Lk);
  const int nsub = kvl.nsub;

  // DMA descriptors: K in the row image, V in the transposing image
  const TilePieces<NPC> pcs = tile_pieces<IMG_ROW, IMG_TR, NPC, NTS>(tis, C, head);
  const i32x4 rs_k = make_rsrc((const bf16*)a.k + (size_t)b * (a.k_bstride ? (size_t)a.k_bstride : (size_t)Lk * C), Lk * C * 2);
  const i32x4 rs_v = make_rsrc((const bf16*)a.v + (size_t)b * (a.v_bstride ? (size_t)a.v_bstride : (size_t)Lk * C), Lk * C * 2);
  const unsigned lds0 = (unsigned)(size_t)(lds_void_t*)smem;
  auto issue = [&](int key0, int bsel) __attribute__((always_inline)) {
    tile_issue<NPC, NTS>(pcs, rs_k, rs_v, key0, Lk, C, __builtin_amdgcn_readfirstlane(lds0 + (st * 2 + bsel) * 2 * TB + qwv * 1024));
  };
  // fragment addresses
  const int kb0 = row_frag_base(r, h, row_image(r));                     // K rows kt*32 + r
  const TrLane vt = tr_lane(lane);                                       // V^T

  int bsel = 0;
  const int sub0 = (nsp == 1) ? 0 : (int)((long long)nsub * sp / nsp);                    // this split's tiles
  const int sub1 = (nsp == 1) ? nsub : (int)((long long)nsub * (sp + 1) / nsp);
  if (sub0 + st < sub1) issue(kvl.start(sub0 + st), 0);
  const int niter = (sub1 - sub0 + KS - 1) / KS;
#pragma unroll 1
  for (int it = 0; it < niter; ++it) {
    const int idx = sub0 + it * KS + st;
    const bool act = idx < sub1;
    const int key0 = act ? kvl.start(idx) : 0;
    dma_wait();
    __syncthreads();                               // tile idx has landed for everybody; buffer bsel^1 is free again
    if (idx + KS < sub1) issue(kvl.start(idx + KS), bsel ^ 1);
    const unsigned char* Kt = smem + (st * 2 + bsel) * 2 * TB;
    const unsigned char* Vt = Kt + TB;
    bsel ^= 1;
    if (!act) continue;
    int cls = (key0 >= Lk) ? 0 : classify<MODE>(qw0, qw0 + 31, key0, key0 + 63, d.pshift, a.T, d.qf_off);
    if (key0 + 63 >= Lk && cls == 2) cls = 1;
    if (cls == 0 || qw0 >= Lq) continue;

    // all fragment reads of the tile go out first (K row fragments, then the transposed V fragments): the V reads
    // complete under the S MFMAs and the softmax, nothing in the chain below waits for LDS
    bf16x8 kf[2][4], vf[2][2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) row_frag(kf[kt], Kt, kb0, kt * 4096);
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) vf[kt][s2][dt] = tr_read(Vt, vt, kt * 32 + 16 * s2, dt);
    f32x16 s[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int i = 0; i < 16; ++i) s[kt][i] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) s[kt] = mfma32(kf[kt][ks], qf[ks], s[kt]);
    }
    // two straight-line versions (one uniform branch per tile): fully allowed tiles carry no mask code at all
    auto softmax = [&](auto masked_) __attribute__((always_inline)) {
      constexpr bool MASKED = decltype(masked_)::value;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          float p = __builtin_amdgcn_exp2f(s[kt][rr] - SOFTMAX_OFF);            // (q carries log2(e)/8: qkv_norm_kernel)
          if constexpr (MASKED) {
            const int key = key0 + kt * 32 + mfma_row(rr, lane);
            if (key >= Lk || !tok_allowed<MODE>(qrow, key, d.pshift, a.T, d.qf_off)) p = 0.f;
          }
          s[kt][rr] = p;
          l2[rr & 1] += p;
        }
    };
    if (cls == 2) softmax(std::false_type{});
    else softmax(std::true_type{});
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 pb = pack8(s[kt], s2);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) o[dt] = mfma32(vf[kt][s2][dt], pb, o[dt]);     // O^T[dv][q] += V^T[dv][key] P^T[key][q]
      }
  }
  float l = l2[0] + l2[1];
  if constexpr (KS > 1) {                          // streams 1 .. KS-1 hand their partial (O, l) to stream 0 through LDS
    float* red = (float*)smem;                     // [KS - 1][QW][33][64] floats
    __syncthreads();
    if (st >= 1) {
      float* rw = red + (size_t)((st - 1) * QW + qwv) * 33 * 64;
#pragma unroll
      for (int i = 0; i < 16; ++i) { rw[i * 64 + lane] = o[0][i]; rw[(16 + i) * 64 + lane] = o[1][i]; }
      rw[32 * 64 + lane] = l;
    }
    __syncthreads();
    if (st != 0) return;
#pragma unroll
    for (int s_ = 0; s_ < KS - 1; ++s_) {
      const float* rr_ = red + (size_t)(s_ * QW + qwv) * 33 * 64;
#pragma unroll
      for (int i = 0; i < 16; ++i) { o[0][i] += rr_[i * 64 + lane]; o[1][i] += rr_[(16 + i) * 64 + lane]; }
      l += rr_[32 * 64 + lane];
    }
  }
  if (qrow >= Lq) return;
  l += __shfl_xor(l, 32);                          // the other half of the keys of every tile lives in lane ^ 32
  if (nsp > 1) {                                   // partial of this split: [split][b][head][q][64 channels | l] fp32
    float* pw = a.split_ws + ((((size_t)sp * a.B + b) * a.heads + head) * Lq + qrow) * 65;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)                   // (rows of 65 floats: not 16-byte aligned, scalar stores)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int k = 0; k < 4; ++k) pw[lane_row_ch(dt, g, h) + k] = o[dt][4 * g + k];
    if (h == 0) pw[64] = l;
    return;
  }
  const float inv = (l > 0.f) ? 1.f / l : 0.f;
  lane_row_store((bf16*)a.out + ((size_t)b * Lq + qrow) * C + head * 64, o, inv, h);
  if (a.lse && h == 0) a.lse[(size_t)(b * a.heads + head) * Lq + qrow] = SOFTMAX_OFF + log2f(fmaxf(l, 1e-30f));
#endif
}

// out[b][q][head*64 + c] = sum_s O_s / sum_s l_s over the kv_splits partials of attn_fwd_kernel (one thread per (b, head, q, 8 channels))
__global__ void attn_split_reduce_kernel(const float* __restrict__ ws, bf16* __restrict__ out, float* __restrict__ lse, int nsp,
                                         int B, int heads, int Lq, int C) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int part = (int)(gid & 7);
  const long long row = gid >> 3;                  // (b * heads + head) * Lq + q
  if (row >= (long long)B * heads * Lq) return;
  const int q = (int)(row % Lq), head = (int)((row / Lq) % heads), b = (int)(row / ((long long)Lq * heads));
  float acc[8], l = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  const size_t plane = (size_t)B * heads * Lq * 65;
  for (int s_ = 0; s_ < nsp; ++s_) {
    const float* p = ws + (size_t)s_ * plane + (size_t)row * 65;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += p[part * 8 + i];
    l += p[64];
  }
  const float inv = (l > 0.f) ? 1.f / l : 0.f;
  bf16x8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = f2bf(acc[i] * inv);
  *(bf16x8*)(out + ((size_t)b * Lq + q) * C + head * 64 + part * 8) = o;
  if (lse && part == 0) lse[row] = SOFTMAX_OFF + log2f(fmaxf(l, 1e-30f));
}

#include <cstdlib>
#include "attention_ws.h"
#include "attention_frame.h"

// ================================================================================================================
// backward: dQ   (the forward's structure: lane = query row, LDS-DMA double-buffered K / V tiles, KS key streams
// whose partial dQ add up in LDS).  K is read both row-wise (S^T = K.Q^T) and transposed (dQ^T += K^T.dS^T): it is
// staged once, in the dual-use image of attention_parts.h (conflict-free for both kinds of read); V is only read
// row-wise (dP^T = V.dO^T).
template <int MODE, int KS>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(const AttnDev d) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int TB = 64 * 128;
  constexpr int QW = 4 / KS, NTS = 64 * QW, NPC = 512 / NTS;
  __shared__ __attribute__((aligned(16))) unsigned char smem[KS * 2 * 2 * TB];     // [stream][buffer][K | V]
  const OnirisAttnArgs& a = d.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 31, h = lane >> 5;
  const int qwv = wave % QW, st = wave / QW, tis = tid % NTS;
  const int nqb = gridDim.x;
  int bx_, head, b;
  attn_block_decode(bx_, head, b);
  const int qbw = nqb - 1 - bx_;
  const int C = a.C, Lq = a.Lq, Lk = a.Lk;
  const int qw0 = qbw * (32 * QW) + qwv * 32;
  const int qrow = qw0 + r;
  const int qb = (qbw * (32 * QW)) >> 7;

  const bf16* qg = (const bf16*)a.q + (size_t)b * Lq * C + head * 64;
  const bf16* dog = (const bf16*)a.dout + (size_t)b * Lq * C + head * 64;
  bf16x8 qf[4], dof[4];
  own_row(qf, qg + (size_t)qrow * C + h * 8, qrow < Lq);
  own_row(dof, dog + (size_t)qrow * C + h * 8, qrow < Lq);
  float lse = 0.f, delta = 0.f;
  if (qrow < Lq) {
    lse = a.lse[(size_t)(b * a.heads + head) * Lq + qrow];
    delta = a.delta[(size_t)(b * a.heads + head) * Lq + qrow];
  }
  asm volatile("" ::"v"(lse), "v"(delta));         // consume the ordinary loads before any LDS-DMA is in flight
  f32x16 dq[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) { dq[0][i] = 0.f; dq[1][i] = 0.f; }

  const BlockList kvl = block_list(a.kv_num, a.kv_idx, a.tab_cols, qb >> d.tshift, d.tshift, lane, Lk);
  const int nsub = kvl.nsub;

  // K is read row-wise (S^T) AND transposed (dQ^T): the dual-use image; V: the row image
  const TilePieces<NPC> pcs = tile_pieces<IMG_DUAL, IMG_ROW, NPC, NTS>(tis, C, head);
  const i32x4 rs_k = make_rsrc((const bf16*)a.k + (size_t)b * Lk * C, Lk * C * 2);
  const i32x4 rs_v = make_rsrc((const bf16*)a.v + (size_t)b * Lk * C, Lk * C * 2);
  const unsigned lds0 = (unsigned)(size_t)(lds_void_t*)smem;
  auto issue = [&](int key0, int bsel) __attribute__((always_inline)) {
    tile_issue<NPC, NTS>(pcs, rs_k, rs_v, key0, Lk, C, __builtin_amdgcn_readfirstlane(lds0 + (st * 2 + bsel) * 2 * TB + qwv * 1024));
  };
  // fragment addresses: row reads of K (dual-use image) and V (row image), rows kt*32 + r; transposing reads of K
  const int kr0 = row_frag_base(r, h, dual_image(r));
  const int vr0 = row_frag_base(r, h, row_image(r));
  const DualLane ktl = dual_lane(lane);

  int bsel = 0;
  if (st < nsub) issue(kvl.start(st), 0);
  const int niter = (nsub + KS - 1) / KS;
#pragma unroll 1
  for (int it = 0; it < niter; ++it) {
    const int idx = it * KS + st;
    const bool act = idx < nsub;
    const int key0 = act ? kvl.start(idx) : 0;
    dma_wait();
    __syncthreads();
    if (idx + KS < nsub) issue(kvl.start(idx + KS), bsel ^ 1);
    const unsigned char* Kt = smem + (st * 2 + bsel) * 2 * TB;
    const unsigned char* Vt = Kt + TB;
    bsel ^= 1;
    if (!act) continue;
    int cls = (key0 >= Lk) ? 0 : classify<MODE>(qw0, qw0 + 31, key0, key0 + 63, d.pshift, a.T, d.qf_off);
    if (key0 + 63 >= Lk && cls == 2) cls = 1;
    if (cls == 0 || qw0 >= Lq) continue;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      bf16x8 kf[4], vf[4], ktf[2][2];
      row_frag2(kf, vf, Kt, kr0, Vt, vr0, kt * 4096);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) ktf[s2][dt] = dual_read(Kt, ktl, kt * 32 + 16 * s2, dt);
      f32x16 s, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s = mfma32(kf[ks], qf[ks], s);
        dp = mfma32(vf[ks], dof[ks], dp);
      }
      auto dsoft = [&](auto masked_) __attribute__((always_inline)) {
        constexpr bool MASKED = decltype(masked_)::value;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          float p = __builtin_amdgcn_exp2f(s[rr] - lse);                     // (q carries log2(e)/8: qkv_norm_kernel)
          if constexpr (MASKED) {
            const int key = key0 + kt * 32 + mfma_row(rr, lane);
            if (key >= Lk || !tok_allowed<MODE>(qrow, key, d.pshift, a.T, d.qf_off)) p = 0.f;
          }
          s[rr] = p * (dp[rr] - delta);                   // dS (the 1/8 of the score scale is applied to dQ in the epilogue)
        }
      };
      if (cls == 2) dsoft(std::false_type{});
      else dsoft(std::true_type{});
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 db = pack8(s, s2);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) dq[dt] = mfma32(ktf[s2][dt], db, dq[dt]);     // dQ^T[d][q] += K^T[d][key] dS^T[key][q]
      }
    }
  }
  if constexpr (KS > 1) {
    float* red = (float*)smem;                     // [QW][32][64] floats
    __syncthreads();
    if (st == 1) {
#pragma unroll
      for (int i = 0; i < 16; ++i) { red[(qwv * 32 + i) * 64 + lane] = dq[0][i]; red[(qwv * 32 + 16 + i) * 64 + lane] = dq[1][i]; }
    }
    __syncthreads();
    if (st != 0) return;
#pragma unroll
    for (int i = 0; i < 16; ++i) { dq[0][i] += red[(qwv * 32 + i) * 64 + lane]; dq[1][i] += red[(qwv * 32 + 16 + i) * 64 + lane]; }
  }
  if (qrow >= Lq) return;
  lane_row_store((bf16*)a.dq + ((size_t)b * Lq + qrow) * C + head * 64, dq, 0.125f, h);
#endif
}

// ================================================================================================================
// backward: dK, dV   (lane = key).  Q / dO tiles (64 queries) and the tile's lse / delta go global -> LDS by LDS-DMA
// into two alternating buffers (one barrier per tile); both tiles are read row-wise (S = Q.K^T, dP = dO.V^T) and
// transposed (dK^T += Q^T.dS, dV^T += dO^T.P) and carry the transposing-read swizzle.
template <int MODE>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_kernel(const AttnDev d) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int TB = 64 * 128, BUFB = 2 * TB + 512;        // Q | dO | lse[64] delta[64]
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BUFB];
  const OnirisAttnArgs& a = d.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 31, h = lane >> 5;
  const int nch = a.dkv_chunks > 1 ? a.dkv_chunks : 1;      // query-list chunks per key block (see OnirisAttnArgs)
  int bx_, head, b;
  attn_block_decode(bx_, head, b);
  const int kb = bx_ / nch, chunk = bx_ % nch;
  const int C = a.C, Lq = a.Lq, Lk = a.Lk;
  const int kw0 = kb * 128 + wave * 32;
  const int krow = kw0 + r;

  const bf16* kg = (const bf16*)a.k + (size_t)b * Lk * C + head * 64;
  const bf16* vg = (const bf16*)a.v + (size_t)b * Lk * C + head * 64;
  bf16x8 kf[4], vf[4];
  own_row(kf, kg + (size_t)krow * C + h * 8, krow < Lk);
  own_row(vf, vg + (size_t)krow * C + h * 8, krow < Lk);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) asm volatile("" ::"v"(kf[ks]), "v"(vf[ks]));    // consume the ordinary loads before any LDS-DMA is in flight
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) { dk[0][i] = 0.f; dk[1][i] = 0.f; dv[0][i] = 0.f; dv[1][i] = 0.f; }

  const BlockList qvl = block_list(a.q_num, a.q_idx, a.qtab_cols, kb >> d.tshift, d.tshift, lane, Lq);     // the key block's query list
  const int nsub = qvl.nsub;

  const TilePieces<2> pcs = tile_pieces<IMG_TR, IMG_TR, 2, 256>(tid, C, head);      // Q and dO: the transposing image
  const i32x4 rs_q = make_rsrc((const bf16*)a.q + (size_t)b * Lq * C, Lq * C * 2);
  const i32x4 rs_do = make_rsrc((const bf16*)a.dout + (size_t)b * Lq * C, Lq * C * 2);
  const i32x4 rs_l = make_rsrc(a.lse + (size_t)(b * a.heads + head) * Lq, Lq * 4);
  const i32x4 rs_d = make_rsrc(a.delta + (size_t)(b * a.heads + head) * Lq, Lq * 4);
  const unsigned lds0 = (unsigned)(size_t)(lds_void_t*)smem;
  auto issue = [&](int q0, int bsel) __attribute__((always_inline)) {
    const int left = Lq - q0;
    tile_issue<2, 256>(pcs, rs_q, rs_do, q0, Lq, C, __builtin_amdgcn_readfirstlane(lds0 + bsel * BUFB + wave * 1024));
    if (wave == 0) {                               // lanes 0..15: lse[q0..q0+63], lanes 16..31: delta (16 B per lane)
      const unsigned sdst = __builtin_amdgcn_readfirstlane(lds0 + bsel * BUFB + 2 * TB);
      const int l16 = lane & 15;
      const int vo = (l16 * 4 < left) ? l16 * 16 : OOB;
      if (lane < 16) dma16(rs_l, vo, q0 * 4, sdst);
      else if (lane < 32) dma16(rs_d, vo, q0 * 4, sdst);
    }
  };
  // row fragments (rows qt*32 + r, 4-way conflict with this swizzle) and transposed fragments
  const int rr0 = row_frag_base(r, h, tr_image(r));
  const TrLane ttl = tr_lane(lane);

  const int i0 = (int)((long long)nsub * chunk / nch), i1 = (int)((long long)nsub * (chunk + 1) / nch);
  int bsel = 0;
  if (i0 < i1) issue(qvl.start(i0), 0);
#pragma unroll 1
  for (int idx = i0; idx < i1; ++idx) {
    const int q0 = qvl.start(idx);
    dma_wait();
    __syncthreads();
    if (idx + 1 < i1) issue(qvl.start(idx + 1), bsel ^ 1);
    const unsigned char* Qt = smem + bsel * BUFB;
    const unsigned char* dOt = Qt + TB;
    const float* lse_lds = (const float*)(Qt + 2 * TB);
    const float* del_lds = lse_lds + 64;
    bsel ^= 1;
    if (kw0 >= Lk || q0 >= Lq) continue;
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const int qq0 = q0 + qt * 32;
      int cls = classify<MODE>(qq0, qq0 + 31, kw0, kw0 + 31, d.pshift, a.T, d.qf_off);
      if ((qq0 + 31 >= Lq || kw0 + 31 >= Lk) && cls == 2) cls = 1;
      if (cls == 0 || qq0 >= Lq) continue;
      bf16x8 qa[4], da[4], dotf[2][2], qtf[2][2];
      row_frag2(qa, da, Qt, rr0, dOt, rr0, qt * 4096);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dotf[s2][dt] = tr_read(dOt, ttl, qt * 32 + 16 * s2, dt);
          qtf[s2][dt] = tr_read(Qt, ttl, qt * 32 + 16 * s2, dt);
        }
      f32x16 s, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s = mfma32(qa[ks], kf[ks], s);                   // S[q][key]
        dp = mfma32(da[ks], vf[ks], dp);                 // dP[q][key]
      }
      f32x16 pv;
      auto dsoft = [&](auto masked_) __attribute__((always_inline)) {
        constexpr bool MASKED = decltype(masked_)::value;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int qb4 = qt * 32 + 8 * g4 + 4 * h;          // 4 consecutive query rows per accumulator group
          const float4 ls = *(const float4*)(lse_lds + qb4), de = *(const float4*)(del_lds + qb4);
          const float lsv[4] = {ls.x, ls.y, ls.z, ls.w}, dev[4] = {de.x, de.y, de.z, de.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int rr = 4 * g4 + k;
            float p = __builtin_amdgcn_exp2f(s[rr] - lsv[k]);                // (q carries log2(e)/8: qkv_norm_kernel)
            if constexpr (MASKED) {
              const int qtok = q0 + qb4 + k;
              if (qtok >= Lq || krow >= Lk || !tok_allowed<MODE>(qtok, krow, d.pshift, a.T, d.qf_off)) p = 0.f;
            }
            pv[rr] = p;
            s[rr] = p * (dp[rr] - dev[k]) * 0.125f;          // dS (scaled)
          }
        }
      };
      if (cls == 2) dsoft(std::false_type{});
      else dsoft(std::true_type{});
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 pb = pack8(pv, s2);
        const bf16x8 db = pack8(s, s2);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dv[dt] = mfma32(dotf[s2][dt], pb, dv[dt]);     // dV^T[dv][key] += dO^T[dv][q] P[q][key]
          dk[dt] = mfma32(qtf[s2][dt], db, dk[dt]);      // dK^T[d][key]  += Q^T[d][q] dS[q][key]
        }
      }
    }
  }
  if (krow >= Lk) return;
  if (nch > 1) {                                     // fp32 partial sums of this chunk (added by attn_dkv_reduce_kernel)
    const size_t plane = (size_t)nch * a.B * Lk * C;
    float* pk = a.dkv_part + (((size_t)chunk * a.B + b) * Lk + krow) * C + head * 64;
    float* pv = pk + plane;
    lane_row_store_f32(pk, dk, h);
    lane_row_store_f32(pv, dv, h);
    return;
  }
  lane_row_store((bf16*)a.dk + ((size_t)b * Lk + krow) * C + head * 64, dk, 1.f / SCALE_LOG2, h);      // dK^T was summed against q' = c q
  lane_row_store((bf16*)a.dv + ((size_t)b * Lk + krow) * C + head * 64, dv, 1.f, h);
#endif
}

#include "attention_bwd_ws.h"
#include "attention_bwd_dq_ws.h"

// dk|dv = sum over the chunks (in chunk order) of the fp32 partials; 8 elements per thread
__global__ void attn_dkv_reduce_kernel(const float* __restrict__ part, bf16* __restrict__ dk, bf16* __restrict__ dv,
                                       size_t n8, int nch) {      // (dk partials were summed against q' = c q: * 1/c here)
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * n8) return;
  const int which = i >= n8;
  const size_t e = (which ? i - n8 : i) * 8;
  const size_t n = n8 * 8;
  const float* p = part + (size_t)which * nch * n + e;
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  for (int c = 0; c < nch; ++c) {
    const float4 u = *(const float4*)(p + (size_t)c * n), w = *(const float4*)(p + (size_t)c * n + 4);
    acc[0] += u.x; acc[1] += u.y; acc[2] += u.z; acc[3] += u.w;
    acc[4] += w.x; acc[5] += w.y; acc[6] += w.z; acc[7] += w.w;
  }
  const float sc = which ? 1.f : (1.f / SCALE_LOG2);
  bf16x8 o;
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = f2bf(acc[k] * sc);
  *(bf16x8*)((which ? dv : dk) + e) = o;
}

// ================================================================================================================
// the prologue of attention: q | k | v normalisation, rotary embedding, KV-ring placement and their adjoints
#include "attention_qkv.h"

// ================================================================================================================
// host entry points
static int ilog2_exact(int v) {
  int s = 0;
  while ((1 << s) < v) ++s;
  return ((1 << s) == v) ? s : -1;
}

static int attn_prepare(const OnirisAttnArgs* args, AttnDev& d, const char* who) {
  if (!args) { oniris_set_error("%s: null args", who); return ONIRIS_EINVAL; }
  d.a = *args;
  const OnirisAttnArgs& a = d.a;
  if (!(a.B > 0 && a.heads > 0 && a.Lq > 0 && a.Lk > 0 && a.C == a.heads * 64)) {
    oniris_set_error("%s: bad sizes (C must be heads*64)", who); return ONIRIS_EINVAL;
  }
  if (a.Lk % 8 != 0 || a.Lq % 8 != 0) { oniris_set_error("%s: Lq, Lk must be multiples of 8", who); return ONIRIS_EINVAL; }
  d.pshift = 0; d.qf_off = 0; d.tshift = 0;
  if (a.kv_num || a.q_num) {
    const int tb = a.tab_block > 0 ? a.tab_block : 128;
    d.tshift = (tb % 128 == 0) ? ilog2_exact(tb / 128) : -1;
    if (d.tshift < 0) { oniris_set_error("%s: table block %d must be 128 * 2^k", who, tb); return ONIRIS_EUNSUPPORTED; }
  }
  if (a.mask_mode != 0) {
    d.pshift = ilog2_exact(a.P);
    if (d.pshift < 0) { oniris_set_error("%s: P=%d must be a power of two", who, a.P); return ONIRIS_EUNSUPPORTED; }
    if (a.mask_mode == 1) {                          // frames appended behind cached ones: the queries are the LAST Lq / P frames
      ONIRIS_CHECK_ARG(a.Lk >= a.Lq && (a.Lk - a.Lq) % a.P == 0,
                       "%s: the frame-causal mask needs Lk >= Lq and whole frames between them (Lq %d, Lk %d, P %d)", who, a.Lq, a.Lk, a.P);
      d.qf_off = (a.Lk - a.Lq) / a.P;
    }
    if (a.mask_mode == 2 && (a.Lq != a.Lk || a.Lq != 2 * a.T * a.P || (a.T * a.P) % 128 != 0)) {
      oniris_set_error("%s: training mask needs Lq == Lk == 2*T*P and T*P %% 128 == 0", who); return ONIRIS_EINVAL;
    }
  }
  if (a.mask_mode < 0 || a.mask_mode > 2) { oniris_set_error("%s: bad mask_mode", who); return ONIRIS_EINVAL; }
  return ONIRIS_OK;
}

#define ATTN_DISPATCH(KERN, GRID)                                                                     \
  switch (d.a.mask_mode) {                                                                            \
    case 0: ONIRIS_KLAUNCH(KERN<0>, GRID, dim3(256), 0, stream, d); break;                        \
    case 1: ONIRIS_KLAUNCH(KERN<1>, GRID, dim3(256), 0, stream, d); break;                        \
    default: ONIRIS_KLAUNCH(KERN<2>, GRID, dim3(256), 0, stream, d); break;                       \
  }

extern "C" int oniris_attn_fwd(const OnirisAttnArgs* args, oniris_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AttnDev d;
  int rc = attn_prepare(args, d, "attn_fwd");
  if (rc) return rc;
  ONIRIS_CHECK_ARG(d.a.q && d.a.k && d.a.v && d.a.out, "attn_fwd: null pointer");
  ONIRIS_CHECK_ARG(d.a.v_bstride == 0 || (!d.a.sched && d.a.v_bstride >= (int64_t)d.a.Lk * d.a.C),
                   "attn_fwd: v_bstride is served by the grid kernel only and must cover a sequence");
  ONIRIS_CHECK_ARG(d.a.k_bstride == 0 || (!d.a.sched && d.a.k_bstride >= (int64_t)d.a.Lk * d.a.C),
                   "attn_fwd: k_bstride is served by the grid kernel only and must cover a sequence");
  if (d.a.sched) {                                  // persistent, statically balanced, wave-specialised kernel (attention_ws.h)
    ONIRIS_CHECK_ARG(d.a.sched_wgs > 0 && d.a.sched_slots > 0, "attn_fwd: empty schedule");
    ONIRIS_CHECK_ARG(d.a.mask_mode != 0, "attn_fwd: the scheduled kernel serves the table-driven masks");
    ONIRIS_CHECK_ARG(d.a.kv_num && d.a.kv_idx && d.a.tab_cols <= 64, "attn_fwd: the scheduled kernel needs a table with <= 64 blocks per row");
    // the kernel's assumptions (only the LAST listed block of a table row is partially masked; 128-row query blocks):
    // true for the DART training table (Lq == Lk == 2*T*P) and for the causal prefill table (Lq == Lk), nothing else
    ONIRIS_CHECK_ARG(d.a.Lq % 128 == 0 && d.a.Lq == d.a.Lk,
                     "attn_fwd: the scheduled kernel needs Lq == Lk, a multiple of 128 (got %d, %d): launch without a schedule",
                     d.a.Lq, d.a.Lk);
    if (d.a.mask_mode == 1) oniris_launch(attn_fwd_ws_kernel<1>, dim3(d.a.sched_wgs), dim3(512), stream, d);
    else oniris_launch(attn_fwd_ws_kernel<2>, dim3(d.a.sched_wgs), dim3(512), stream, d);
    ONIRIS_LAUNCH_CHECK();
    return ONIRIS_OK;
  }
  if (frame_attn_ok(d.a)) {                          // dense attention inside frames of 64 / 128 / 256 tokens (attention_frame.h)
    FrameAttnDev f{d.a, (long long)d.a.B * d.a.Lq, d.a.Lq / 64};
    ONIRIS_CHECK_ARG((f.ntok + 255) / 256 < (1LL << 31), "attn_fwd: too many tokens");
    const long long nsb = (f.ntok + 255) / 256;
    if (d.a.Lq == 256 && nsb * d.a.heads <= 64 && !(d.a.frame_kernel & 4))         // few 256-token frames: two query halves per frame
      oniris_launch(frame_attn_fwd_kernel<1>, dim3((unsigned)(2 * nsb), d.a.heads), dim3(256), stream, f);
    else
      oniris_launch(frame_attn_fwd_kernel<2>, dim3((unsigned)nsb, d.a.heads), dim3(256), stream, f);
    ONIRIS_LAUNCH_CHECK();
    return ONIRIS_OK;
  }
  // two key streams per workgroup (64 query rows) when the key lists are long and causal, else one (128 rows)
  const bool split = d.a.mask_mode != 0 && d.a.Lk >= 2048;
  if (d.a.kv_splits > 1) {                           // split-KV decode: partials + reduction (two launches)
    ONIRIS_CHECK_ARG(d.a.mask_mode == 0 && d.a.split_ws && d.a.kv_splits <= 256,
                     "attn_fwd: kv_splits serves the dense (mask_mode 0) kernel and needs split_ws");
    const dim3 gs(cdiv(d.a.Lq, 128) * d.a.kv_splits, d.a.heads, d.a.B);
    ONIRIS_KLAUNCH((attn_fwd_kernel<0, 1>), gs, dim3(256), 0, stream, d);
    ONIRIS_LAUNCH_CHECK();
    const long long nthr = (long long)d.a.B * d.a.heads * d.a.Lq * 8;
    ONIRIS_KLAUNCH(attn_split_reduce_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, stream,
                       (const float*)d.a.split_ws, (bf16*)d.a.out, d.a.lse, d.a.kv_splits, d.a.B, d.a.heads, d.a.Lq, d.a.C);
    ONIRIS_LAUNCH_CHECK();
    return ONIRIS_OK;
  }
  // decode of a frame against a short ring (below the split-KV threshold): a handful of workgroups, each a serial walk over the key
  // tiles (~0.5 us per tile: 13 us per layer at 18 cached frames, three times the launch floor) -- four key streams per workgroup
  // of 32 query rows cut that walk by four inside ONE launch (round 6)
  if (d.a.mask_mode == 0 && !(d.a.frame_kernel & 2) && d.a.Lk >= 256 && d.a.Lk > d.a.Lq &&
      (long long)cdiv(d.a.Lq, 32) * d.a.heads * d.a.B <= 512) {
    ONIRIS_KLAUNCH((attn_fwd_kernel<0, 4>), dim3(cdiv(d.a.Lq, 32), d.a.heads, d.a.B), dim3(256), 0, stream, d);
    ONIRIS_LAUNCH_CHECK();
    return ONIRIS_OK;
  }
  const dim3 grid(cdiv(d.a.Lq, split ? 64 : 128), d.a.heads, d.a.B);
  if (split) {
    if (d.a.mask_mode == 1) ONIRIS_KLAUNCH((attn_fwd_kernel<1, 2>), grid, dim3(256), 0, stream, d);
    else ONIRIS_KLAUNCH((attn_fwd_kernel<2, 2>), grid, dim3(256), 0, stream, d);
  } else {
    switch (d.a.mask_mode) {
      case 0: ONIRIS_KLAUNCH((attn_fwd_kernel<0, 1>), grid, dim3(256), 0, stream, d); break;
      case 1: ONIRIS_KLAUNCH((attn_fwd_kernel<1, 1>), grid, dim3(256), 0, stream, d); break;
      default: ONIRIS_KLAUNCH((attn_fwd_kernel<2, 1>), grid, dim3(256), 0, stream, d); break;
    }
  }
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_attn_bwd_dq(const OnirisAttnArgs* args, oniris_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AttnDev d;
  int rc = attn_prepare(args, d, "attn_bwd_dq");
  if (rc) return rc;
  ONIRIS_CHECK_ARG(d.a.q && d.a.k && d.a.v && d.a.dout && d.a.lse && d.a.delta && d.a.dq,
                   "attn_bwd_dq: null pointer");
  if (d.a.sched) {                                  // persistent, statically balanced, wave-specialised kernel (attention_bwd_dq_ws.h):
    // the forward's work list (query blocks of 128 rows); lse / delta point at the NEGATED rows (oniris_attn_bwd_prep)
    ONIRIS_CHECK_ARG(d.a.mask_mode != 0 && d.a.kv_num && d.a.kv_idx && d.a.tab_cols <= 64 && d.a.sched_wgs > 0 && d.a.sched_slots > 0,
                     "attn_bwd_dq: the scheduled kernel needs a table-driven mask with <= 64 blocks per row");
    ONIRIS_CHECK_ARG(d.a.Lq % 128 == 0 && d.a.Lq == d.a.Lk && d.a.Lq / 128 < 65536,
                     "attn_bwd_dq: the scheduled kernel needs Lq == Lk, a multiple of 128 (got %d, %d)", d.a.Lq, d.a.Lk);
    // mask_mode 1 + a block-diagonal table = dense attention inside every frame (FrameAttention with P = 128 * 2^k tokens)
    if (d.a.mask_mode == 1) oniris_launch(attn_bwd_dq_ws_kernel<1>, dim3(d.a.sched_wgs), dim3(512), stream, d);
    else oniris_launch(attn_bwd_dq_ws_kernel<2>, dim3(d.a.sched_wgs), dim3(512), stream, d);
    ONIRIS_LAUNCH_CHECK();
    return ONIRIS_OK;
  }
  if (frame_attn_ok(d.a)) {                          // dense attention inside frames of 64 / 128 / 256 tokens (attention_frame.h)
    FrameAttnDev f{d.a, (long long)d.a.B * d.a.Lq, d.a.Lq / 64};
    oniris_launch(frame_attn_dq_kernel, dim3((unsigned)((f.ntok + 255) / 256), d.a.heads), dim3(256), stream, f);
    ONIRIS_LAUNCH_CHECK();
    return ONIRIS_OK;
  }
  const bool split = d.a.mask_mode != 0 && d.a.Lk >= 2048;
  const dim3 grid(cdiv(d.a.Lq, split ? 64 : 128), d.a.heads, d.a.B);
  if (split) {
    if (d.a.mask_mode == 1) ONIRIS_KLAUNCH((attn_bwd_dq_kernel<1, 2>), grid, dim3(256), 0, stream, d);
    else ONIRIS_KLAUNCH((attn_bwd_dq_kernel<2, 2>), grid, dim3(256), 0, stream, d);
  } else {
    switch (d.a.mask_mode) {
      case 0: ONIRIS_KLAUNCH((attn_bwd_dq_kernel<0, 1>), grid, dim3(256), 0, stream, d); break;
      case 1: ONIRIS_KLAUNCH((attn_bwd_dq_kernel<1, 1>), grid, dim3(256), 0, stream, d); break;
      default: ONIRIS_KLAUNCH((attn_bwd_dq_kernel<2, 1>), grid, dim3(256), 0, stream, d); break;
    }
  }
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_frame_attn_bwd(const OnirisAttnArgs* args, oniris_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AttnDev d;
  int rc = attn_prepare(args, d, "frame_attn_bwd");
  if (rc) return rc;
  ONIRIS_CHECK_ARG(d.a.q && d.a.k && d.a.v && d.a.out && d.a.dout && d.a.lse && d.a.dq && d.a.dk && d.a.dv, "frame_attn_bwd: null pointer");
  OnirisAttnArgs chk = d.a;
  chk.frame_kernel = 0;
  ONIRIS_CHECK_ARG(frame_attn_ok(chk), "frame_attn_bwd: dense attention inside frames of 64 / 128 / 256 tokens only (mask_mode 0, Lq == Lk, "
                                       "no table / schedule / ring strides / split)");
  FrameAttnDev f{d.a, (long long)d.a.B * d.a.Lq, d.a.Lq / 64};
  ONIRIS_CHECK_ARG((f.ntok + 255) / 256 < (1LL << 31), "frame_attn_bwd: too many tokens");
  oniris_launch(frame_attn_bwd_kernel, dim3((unsigned)((f.ntok + 255) / 256), d.a.heads), dim3(512), stream, f);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

static int frame_qkv_dev(FrameQkvDev& f, const void* qkv, void* out, float* lse, const void* dout, void* dqkv, int64_t n_frames, int P,
                         int heads, const char* who) {
  ONIRIS_CHECK_ARG(qkv && out && lse && n_frames > 0 && heads > 0, "%s: bad arguments", who);
  ONIRIS_CHECK_ARG(P == 64 || P == 128 || P == 256, "%s: frames of 64 / 128 / 256 tokens (got %d)", who, P);
  f.qkv = (const bf16*)qkv; f.out = (bf16*)out; f.lse = lse; f.dout = (const bf16*)dout; f.dqkv = (bf16*)dqkv;
  f.ntok = (long long)n_frames * P; f.P = P; f.heads = heads; f.C = heads * 64; f.tiles = P / 64;
  ONIRIS_CHECK_ARG((f.ntok + 255) / 256 < (1LL << 31) && heads < 65536, "%s: too many tokens", who);
  return ONIRIS_OK;
}

extern "C" int oniris_frame_attn_qkv_fwd(const void* qkv, void* out, float* lse, int64_t n_frames, int P, int heads,
                                         oniris_stream_t stream_) {
  FrameQkvDev f{};
  int rc = frame_qkv_dev(f, qkv, out, lse, nullptr, nullptr, n_frames, P, heads, "frame_attn_qkv_fwd");
  if (rc) return rc;
  oniris_launch(frame_attn_qkv_fwd_kernel, dim3((unsigned)((f.ntok + 255) / 256), heads), dim3(256), (hipStream_t)stream_, f);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

#ifdef FRAME_STAMP
extern "C" int oniris_frame_attn_qkv_fwd_stamp(const void* qkv, void* out, float* lse, void* stamps, int64_t n_frames, int P, int heads,
                                               oniris_stream_t stream_) {
  FrameQkvDev f{};
  int rc = frame_qkv_dev(f, qkv, out, lse, nullptr, stamps, n_frames, P, heads, "frame_attn_qkv_fwd_stamp");
  if (rc) return rc;
  oniris_launch(frame_attn_qkv_fwd_kernel, dim3((unsigned)((f.ntok + 255) / 256), heads), dim3(256), (hipStream_t)stream_, f);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}
#endif

extern "C" int oniris_frame_attn_qkv_bwd(const void* qkv, const void* out, const float* lse, const void* dout, void* dqkv, int64_t n_frames,
                                         int P, int heads, oniris_stream_t stream_) {
  FrameQkvDev f{};
  int rc = frame_qkv_dev(f, qkv, (void*)out, (float*)lse, dout, dqkv, n_frames, P, heads, "frame_attn_qkv_bwd");
  if (rc) return rc;
  ONIRIS_CHECK_ARG(dout && dqkv, "frame_attn_qkv_bwd: dout / dqkv");
  oniris_launch(frame_attn_qkv_bwd_kernel, dim3((unsigned)((f.ntok + 255) / 256), heads), dim3(512), (hipStream_t)stream_, f);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_attn_bwd_dkv(const OnirisAttnArgs* args, oniris_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AttnDev d;
  int rc = attn_prepare(args, d, "attn_bwd_dkv");
  if (rc) return rc;
  ONIRIS_CHECK_ARG(d.a.q && d.a.k && d.a.v && d.a.dout && d.a.lse && d.a.delta && d.a.dk && d.a.dv,
                   "attn_bwd_dkv: null pointer");
  if (d.a.sched) {                                  // persistent, statically balanced, wave-specialised kernel (attention_bwd_ws.h):
    // items = 64-key blocks with their whole query list (schedule built over Lk / 64 items per pair); no partial sums
    ONIRIS_CHECK_ARG(d.a.sched_wgs > 0 && d.a.sched_slots > 0, "attn_bwd_dkv: empty schedule");
    ONIRIS_CHECK_ARG(d.a.mask_mode != 0, "attn_bwd_dkv: the scheduled kernel serves the table-driven masks");
    ONIRIS_CHECK_ARG(d.a.q_num && d.a.q_idx && d.a.qtab_cols <= 64,
                     "attn_bwd_dkv: the scheduled kernel needs the transposed table with <= 64 blocks per row");
    ONIRIS_CHECK_ARG(d.a.Lq % 128 == 0 && d.a.Lq == d.a.Lk && d.a.Lk / 64 < 65536,
                     "attn_bwd_dkv: the scheduled kernel needs Lq == Lk, a multiple of 128 (got %d, %d)", d.a.Lq, d.a.Lk);
    ONIRIS_CHECK_ARG(d.a.dkv_item_keys == 0 || d.a.dkv_item_keys == 64 || d.a.dkv_item_keys == 128,
                     "attn_bwd_dkv: dkv_item_keys is 0 / 64 or 128");
    if (d.a.dkv_item_keys == 128) {
      if (d.a.mask_mode == 1) oniris_launch(attn_bwd_dkv_ws_kernel<1, 128>, dim3(d.a.sched_wgs), dim3(512), stream, d);
      else oniris_launch(attn_bwd_dkv_ws_kernel<2, 128>, dim3(d.a.sched_wgs), dim3(512), stream, d);
    } else {
      if (d.a.mask_mode == 1) oniris_launch(attn_bwd_dkv_ws_kernel<1, 64>, dim3(d.a.sched_wgs), dim3(512), stream, d);
      else oniris_launch(attn_bwd_dkv_ws_kernel<2, 64>, dim3(d.a.sched_wgs), dim3(512), stream, d);
    }
    ONIRIS_LAUNCH_CHECK();
    return ONIRIS_OK;
  }
  const int nch = d.a.dkv_chunks > 1 ? d.a.dkv_chunks : 1;
  ONIRIS_CHECK_ARG(nch == 1 || d.a.dkv_part, "attn_bwd_dkv: dkv_chunks > 1 needs the dkv_part scratch");
  ONIRIS_CHECK_ARG(nch <= 64, "attn_bwd_dkv: at most 64 chunks");
  const dim3 grid(cdiv(d.a.Lk, 128) * nch, d.a.heads, d.a.B);
  ATTN_DISPATCH(attn_bwd_dkv_kernel, grid);
  ONIRIS_LAUNCH_CHECK();
  if (nch > 1) {
    const size_t n8 = (size_t)d.a.B * d.a.Lk * d.a.C / 8;
    ONIRIS_KLAUNCH(attn_dkv_reduce_kernel, dim3((unsigned)((2 * n8 + 255) / 256)), dim3(256), 0, stream,
                       (const float*)d.a.dkv_part, (bf16*)d.a.dk, (bf16*)d.a.dv, n8, nch);
    ONIRIS_LAUNCH_CHECK();
  }
  return ONIRIS_OK;
}

// the kernels of the 8-lane layout (attention_qkv.h): 8 threads per head vector, 256 per workgroup
static long long qkv_nvec(int64_t n_tokens, int C) { return (long long)n_tokens * 3 * C / 64; }
static dim3 lane8_grid(long long nvec) { return dim3((unsigned)((nvec * 8 + 255) / 256)); }

extern "C" int oniris_qkv_norm_rope(const void* qkv, void* q, void* k, void* v, const float* cos_t, const float* sin_t,
                                    const float* scale_t, int64_t n_tokens, int C, int P, int pos_mod, oniris_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ONIRIS_CHECK_ARG(qkv && q && k && v && cos_t && sin_t && scale_t && n_tokens > 0 && C > 0 && C % 64 == 0 && P > 0 && pos_mod > 0,
                   "qkv_norm_rope: bad arguments");
  const long long nvec = qkv_nvec(n_tokens, C);
  ONIRIS_KLAUNCH(qkv_norm_rope_kernel, lane8_grid(nvec), dim3(256), 0, stream, (const bf16*)qkv,
                     (bf16*)q, (bf16*)k, (bf16*)v, cos_t, sin_t, scale_t, nvec, C, P, pos_mod);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_qkv_norm_rope_eval(const void* qkv, void* q, void* k, void* v, void* kr, const float* cos_t,
                                         const float* sin_t, const float* scale_t, int64_t n_tokens, int C,
                                         int64_t kv_tokens_per_batch, int64_t kv_batch_stride, int64_t kv_token_offset, int pos,
                                         oniris_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ONIRIS_CHECK_ARG(qkv && q && k && v && kr && cos_t && sin_t && scale_t && n_tokens > 0 && C % 64 == 0 && pos >= 0 &&
                   kv_tokens_per_batch > 0 && n_tokens % kv_tokens_per_batch == 0 && n_tokens % 8 == 0 &&
                   kv_batch_stride >= (kv_token_offset + kv_tokens_per_batch) * C, "qkv_norm_rope_eval: bad arguments");
  const long long nvec = qkv_nvec(n_tokens, C);
  ONIRIS_KLAUNCH(qkv_norm_rope_eval_kernel, lane8_grid(nvec), dim3(256), 0, stream,
                     (const bf16*)qkv, (bf16*)q, (bf16*)k, (bf16*)v, (bf16*)kr, cos_t, sin_t, scale_t, nvec, C,
                     (long long)kv_tokens_per_batch, (long long)kv_batch_stride, (long long)kv_token_offset, pos);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

static int qkv_eval_impl(const void* x, const void* w, void* q, void* k, void* v, void* kr, const float* cos_t, const float* sin_t,
                         const float* scale_t, int64_t n_tokens, int C, int CinP, int64_t kv_tokens_per_batch,
                         int64_t kv_batch_stride, int64_t kv_token_offset, int pos, int64_t split, void* q2, void* k2, void* v2,
                         hipStream_t stream) {
  ONIRIS_CHECK_ARG(x && w && q && k && v && n_tokens > 0 && C > 0 && C % 64 == 0 && CinP >= C && CinP % 8 == 0 && pos >= 0,
                   "qkv_eval: bad arguments");
  ONIRIS_CHECK_ARG((cos_t && sin_t && scale_t) || (!cos_t && !sin_t && !scale_t && !kr), "qkv_eval: all rotary tables or none");
  ONIRIS_CHECK_ARG(kv_tokens_per_batch == 0 || (kv_tokens_per_batch > 0 && split % kv_tokens_per_batch == 0 &&
                                                kv_batch_stride >= (kv_token_offset + kv_tokens_per_batch) * C),
                   "qkv_eval: bad KV ring geometry");
  const char* tag = split < n_tokens ? "pair-rows" : nullptr;
  // a few tiles (one frame per sequence; at most one workgroup per CU): 32-token tiles, the four waves of a workgroup split the K
  // (qkv_eval_few_kernel; ONIRIS_QKV_EVAL_FEW=0 in the environment: off, A/B)
  static const int qkv_few = getenv("ONIRIS_QKV_EVAL_FEW") ? atoi(getenv("ONIRIS_QKV_EVAL_FEW")) : 1;
  if (qkv_few && ((n_tokens + 31) / 32) * (3LL * C / 64) <= 256) {
    const dim3 gf((unsigned)((n_tokens + 31) / 32), (unsigned)(C / 64), 3u);
    if (oniris_census_on) oniris_census_note((const void*)qkv_eval_few_kernel, tag);
    hipLaunchKernelGGL(qkv_eval_few_kernel, gf, dim3(256), 0, stream, (const bf16*)x, (const bf16*)w, (bf16*)q, (bf16*)k, (bf16*)v,
                       (bf16*)kr, cos_t, sin_t, scale_t, (long long)n_tokens, C, CinP, (long long)kv_tokens_per_batch,
                       (long long)kv_batch_stride, (long long)kv_token_offset, pos, (long long)split, (bf16*)q2, (bf16*)k2, (bf16*)v2);
    ONIRIS_LAUNCH_CHECK();
    return ONIRIS_OK;
  }
  const dim3 grid((unsigned)((n_tokens + 127) / 128), (unsigned)(C / 64), 3u);        // (x: token tile, y: head, z: q | k | v)
#define QKV_EVAL_LAUNCH(KC_)                                                                                              \
  do {                                                                                                                    \
    if (oniris_census_on) oniris_census_note((const void*)qkv_eval_kernel<KC_>, tag);                                     \
    hipLaunchKernelGGL(qkv_eval_kernel<KC_>, grid, dim3(256), 0, stream, (const bf16*)x, (const bf16*)w, (bf16*)q, (bf16*)k, \
                       (bf16*)v, (bf16*)kr, cos_t, sin_t, scale_t, (long long)n_tokens, C, CinP,                          \
                       (long long)kv_tokens_per_batch, (long long)kv_batch_stride, (long long)kv_token_offset, pos,       \
                       (long long)split, (bf16*)q2, (bf16*)k2, (bf16*)v2);                                               \
  } while (0)
  if (C % 256 == 0) QKV_EVAL_LAUNCH(256);
  else if (C % 128 == 0) QKV_EVAL_LAUNCH(128);
  else QKV_EVAL_LAUNCH(64);
#undef QKV_EVAL_LAUNCH
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_qkv_eval(const void* x, const void* w, void* q, void* k, void* v, void* kr, const float* cos_t,
                               const float* sin_t, const float* scale_t, int64_t n_tokens, int C, int CinP,
                               int64_t kv_tokens_per_batch, int64_t kv_batch_stride, int64_t kv_token_offset, int pos,
                               oniris_stream_t stream_) {
  return qkv_eval_impl(x, w, q, k, v, kr, cos_t, sin_t, scale_t, n_tokens, C, CinP, kv_tokens_per_batch, kv_batch_stride,
                       kv_token_offset, pos, n_tokens, nullptr, nullptr, nullptr, (hipStream_t)stream_);
}

extern "C" int oniris_qkv_eval_pair(const void* x, const void* w, void* q, void* k, void* v, void* kr, const float* cos_t,
                                    const float* sin_t, const float* scale_t, int64_t n_tokens, int64_t split, int C, int CinP,
                                    int64_t kv_tokens_per_batch, int64_t kv_batch_stride, int64_t kv_token_offset, int pos,
                                    void* q2, void* k2, void* v2, oniris_stream_t stream_) {
  ONIRIS_CHECK_ARG(split > 0 && split < n_tokens && q2 && k2 && v2, "qkv_eval_pair: need 0 < split < n_tokens and the side buffers");
  return qkv_eval_impl(x, w, q, k, v, kr, cos_t, sin_t, scale_t, n_tokens, C, CinP, kv_tokens_per_batch, kv_batch_stride,
                       kv_token_offset, pos, split, q2, k2, v2, (hipStream_t)stream_);
}

extern "C" int oniris_qkv_norm_rope_bwd(const void* qkv, const void* dq, const void* dk, const void* dv, void* dqkv,
                                        const float* cos_t, const float* sin_t, const float* scale_t, int64_t n_tokens, int C,
                                        int P, int pos_mod, oniris_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ONIRIS_CHECK_ARG(qkv && dq && dk && dv && dqkv && cos_t && sin_t && scale_t && n_tokens > 0 && C > 0 && C % 64 == 0 && P > 0 &&
                   pos_mod > 0, "qkv_norm_rope_bwd: bad arguments");
  const long long nvec = qkv_nvec(n_tokens, C);
  ONIRIS_KLAUNCH(qkv_norm_rope_bwd_kernel, lane8_grid(nvec), dim3(256), 0, stream, (const bf16*)qkv,
                     (const bf16*)dq, (const bf16*)dk, (const bf16*)dv, (bf16*)dqkv, cos_t, sin_t, scale_t, nvec, C, P, pos_mod);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_qkv_norm(const void* qkv, void* q, void* k, void* v, int64_t n_tokens, int C,
                               int64_t kv_tokens_per_batch, int64_t kv_batch_stride, int64_t kv_token_offset,
                               oniris_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ONIRIS_CHECK_ARG(qkv && q && k && v && n_tokens > 0 && C > 0 && C % 64 == 0, "qkv_norm: bad arguments");
  ONIRIS_CHECK_ARG(kv_tokens_per_batch == 0 || (kv_tokens_per_batch > 0 && n_tokens % kv_tokens_per_batch == 0 &&
                   kv_token_offset >= 0 && kv_batch_stride >= (kv_token_offset + kv_tokens_per_batch) * C),
                   "qkv_norm: bad KV ring description");
  const long long nvec = qkv_nvec(n_tokens, C);
  ONIRIS_KLAUNCH(qkv_norm_kernel, lane8_grid(nvec), dim3(256), 0, stream, (const bf16*)qkv,
                     (bf16*)q, (bf16*)k, (bf16*)v, nvec, C, (long long)kv_tokens_per_batch, (long long)kv_batch_stride,
                     (long long)kv_token_offset);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_qkv_norm_bwd(const void* qkv, const void* dq, const void* dk, const void* dv, void* dqkv,
                                   int64_t n_tokens, int C, oniris_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ONIRIS_CHECK_ARG(qkv && dq && dk && dv && dqkv && n_tokens > 0 && C > 0 && C % 64 == 0, "qkv_norm_bwd: bad arguments");
  const long long nvec = qkv_nvec(n_tokens, C);
  ONIRIS_KLAUNCH(qkv_norm_bwd_kernel, lane8_grid(nvec), dim3(256), 0, stream,
                     (const bf16*)qkv, (const bf16*)dq, (const bf16*)dk, (const bf16*)dv, (bf16*)dqkv, nvec, C);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_rope(const void* x, void* xr, void* xt, const float* cos_t, const float* sin_t,
                           const float* scale_t, int mode, int B, int frames, int P, int C, int pos_offset, int pos_mod,
                           int64_t x_batch_stride, int64_t xr_batch_stride, oniris_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ONIRIS_CHECK_ARG(x && (xr || xt) && B > 0 && frames > 0 && P > 0 && C % 64 == 0 && mode >= 0 && mode <= 4,
                   "rope: bad arguments");
  ONIRIS_CHECK_ARG(mode == 0 || (cos_t && sin_t && scale_t && pos_mod > 0), "rope: tables missing");
  const int L = frames * P;
  ONIRIS_CHECK_ARG(L % 8 == 0, "rope: frames*P must be a multiple of 8");
  ONIRIS_CHECK_ARG(x_batch_stride == 0 || x_batch_stride >= (int64_t)L * C, "rope: batch stride smaller than a sequence");
  ONIRIS_CHECK_ARG(xr_batch_stride == 0 || xr_batch_stride >= (int64_t)L * C, "rope: output batch stride smaller than a sequence");
  const dim3 grid(cdiv(L, 64), C / 64, B);
  ONIRIS_KLAUNCH(rope_kernel, grid, dim3(256), 0, stream, (const bf16*)x, (bf16*)xr, (bf16*)xt, cos_t, sin_t,
                     scale_t, mode, L, P, C, C / 64, pos_offset, pos_mod > 0 ? pos_mod : 1,
                     (long long)(x_batch_stride > 0 ? x_batch_stride : (int64_t)L * C),
                     (long long)(xr_batch_stride > 0 ? xr_batch_stride : (int64_t)L * C));
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_attn_bwd_prep(const void* dout, const void* out, float* delta, void* doutt, const float* lse, float* neg,
                                    int B, int heads, int L, int C, oniris_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ONIRIS_CHECK_ARG(dout && out && delta && B > 0 && heads > 0 && L > 0 && C == heads * 64, "attn_bwd_prep: bad arguments");
  ONIRIS_CHECK_ARG(!neg || lse, "attn_bwd_prep: the negated row constants need lse");
  const long long nvec = (long long)B * L * heads;
  ONIRIS_KLAUNCH(attn_delta_kernel, lane8_grid(nvec), dim3(256), 0, stream,
                     (const bf16*)dout, (const bf16*)out, delta, lse, neg, nvec, L, C, heads);
  ONIRIS_LAUNCH_CHECK();
  if (doutt) return oniris_rope(dout, nullptr, doutt, nullptr, nullptr, nullptr, 0, B, L, 1, C, 0, 1, 0, 0, stream_);
  return ONIRIS_OK;
}
