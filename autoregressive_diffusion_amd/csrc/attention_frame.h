// Dense attention INSIDE frames of P = 64 / 128 / 256 tokens, head width 64: FrameAttention (reference
// edm2/attention/attention_modules.py:105-119) and VideoAttention's just_2d branch (:36-45) -- 16x16 latents in the Lunar-Lander
// net, 8x8 in the Counter-Strike net.
//
// Why kernels of their own (round 6).  The grid kernels (attention.hip) give a workgroup 128 query rows and stream the keys in
// 64-row tiles behind one barrier + one LDS-DMA wait each; with 256 keys that is four waits in front of 16 MFMAs per wave each,
// two workgroups per (frame, head) that both copy all of K and V: 0.14-0.19 of the bf16 MFMA peak (profiles/r05_conv_shapes.txt).
// The persistent VideoAttention kernels on a block-diagonal table were measured too (profiles/r06_ab_frame_ws.txt): slower.
// Here a workgroup owns a SUPER-BLOCK of 256 consecutive tokens of one head -- 256 / P whole frames -- whose K | V (forward, dQ)
// or Q | dO (dK / dV) images, 64 KB, land in LDS by ONE burst of LDS-DMA behind ONE barrier; wave w owns rows 64 w .. 64 w + 63
// (two 32-row MFMA blocks that share every fragment read from LDS) and walks the P / 64 tiles of ITS frame.  No mask exists
// (everything inside a frame is allowed), so the hot loop is the unmasked tile body of the grid kernels.
//
// Operand layouts, swizzles (attention_parts.h) and the no-running-maximum softmax are those of attention.hip; q arrives carrying
// log2(e) / 8 (qkv_norm_kernel), lse is log2-domain.
#pragma once

struct FrameAttnDev {
  OnirisAttnArgs a;
  long long ntok;          // B * P tokens per head
  int tiles;               // P / 64: key tiles per frame
};

// one burst of an NT-thread workgroup: tile t (64 rows x 64 channels of head `head`) of tensors g0 / g1 (row pitches C0 / C1) -> LDS
// [t][g0 | g1], swizzled on the source side into the images IMG0 / IMG1 of attention_parts.h.  Every wave issues its copies tile by
// tile: 8 DMA instructions per wave and burst at NT = 512 (the counted wait of the backward kernels relies on it), 16 at NT = 256.
template <int IMG0, int IMG1, int NT>
__device__ __forceinline__ void frame_burst(const bf16* g0, const bf16* g1, long long tok0, long long ntok, int C0, int C1, int head, unsigned lds0,
                                            int tid) {
  constexpr int TB = 64 * 128;
  const int wave = tid >> 6;
  const long long left = ntok - tok0;
  const int rows = left >= 256 ? 256 : (int)left;
  const i32x4 r0 = make_rsrc(g0 + (size_t)tok0 * C0, rows * C0 * 2);
  const i32x4 r1 = make_rsrc(g1 + (size_t)tok0 * C1, rows * C1 * 2);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int i = 0; i < 512 / NT; ++i) {
      const int e = i * NT + tid, row = e >> 3, pp = e & 7;
      const bool ok = t * 64 + row < rows;
      const unsigned dst = lds0 + t * 2 * TB + i * (NT * 16) + wave * 1024;
      dma16(r0, ok ? image_src<IMG0>(row, pp, C0, head) : OOB, t * 64 * C0 * 2, dst);
      dma16(r1, ok ? image_src<IMG1>(row, pp, C1, head) : OOB, t * 64 * C1 * 2, dst + TB);
    }
  }
}

// ---- the tile bodies, once each; the plain kernels and the raw-qkv kernels differ only in what surrounds them -------------------
// lane roles of the forward (K row image, V transposing image) and of the backward passes (K / Q / dO dual-use image, V row image):
// computed by the kernel, where its own address arithmetic sits, and handed to the bodies
struct FrameFwdLane { int kb0; TrLane vt; };
__device__ __forceinline__ FrameFwdLane frame_fwd_lane(int lane) {
  const int r = lane & 31, h = lane >> 5;
  return FrameFwdLane{row_frag_base(r, h, row_image(r)), tr_lane(lane)};
}
struct FrameBwdLane { int kr0, vr0, h; DualLane kt; };
__device__ __forceinline__ FrameBwdLane frame_bwd_lane(int lane) {
  const int r = lane & 31, h = lane >> 5;
  return FrameBwdLane{row_frag_base(r, h, dual_image(r)), row_frag_base(r, h, row_image(r)), h, dual_lane(lane)};
}
// forward: tiles [t0, t0 + tiles) of the staged [tile][K (row image) | V (transposing image)] against J 32-row query blocks of this
// wave (lane = query row); o / l2 accumulate the un-normalised O^T and the two half row sums
template <int J>
__device__ __forceinline__ void frame_fwd_tiles(f32x16 (&o)[J][2], float (&l2)[J][2], const bf16x8 (&qf)[J][4], const unsigned char* smem, int t0,
                                                int tiles, const FrameFwdLane& ln) {
  constexpr int TB = 64 * 128;
  const int kb0 = ln.kb0;
  const TrLane vt = ln.vt;
#pragma unroll 1
  for (int t = t0; t < t0 + tiles; ++t) {
    const unsigned char* Kt = smem + t * 2 * TB;
    const unsigned char* Vt = Kt + TB;
    bf16x8 kf[2][4], vf[2][2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) row_frag(kf[kt], Kt, kb0, kt * 4096);
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) vf[kt][s2][dt] = tr_read(Vt, vt, kt * 32 + 16 * s2, dt);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      f32x16 s[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int i = 0; i < 16; ++i) s[kt][i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) s[kt] = mfma32(kf[kt][ks], qf[j][ks], s[kt]);
      }
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          const float p = __builtin_amdgcn_exp2f(s[kt][rr] - SOFTMAX_OFF);
          s[kt][rr] = p;
          l2[j][rr & 1] += p;
        }
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const bf16x8 pb = pack8(s[kt], s2);
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) o[j][dt] = mfma32(vf[kt][s2][dt], pb, o[j][dt]);
        }
    }
  }
}
// forward epilogue: rows row0 + 32 j (this lane's) of out [tok][C] and of lse [b][head][P] (lse may be null)
template <int J>
__device__ __forceinline__ void frame_fwd_store(const f32x16 (&o)[J][2], const float (&l2)[J][2], long long row0, long long ntok, bf16* out, float* lse,
                                                int C, int P, int heads, int head, int h) {
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const long long qrow = row0 + j * 32;
    float l = l2[j][0] + l2[j][1];
    l += __shfl_xor(l, 32);
    if (qrow >= ntok) continue;
    const float inv = (l > 0.f) ? 1.f / l : 0.f;
    lane_row_store(out + (size_t)qrow * C + head * 64, o[j], inv, h);
    if (lse && h == 0) {
      const long long b = qrow / P;
      lse[(size_t)(b * heads + head) * P + (qrow - b * P)] = SOFTMAX_OFF + log2f(fmaxf(l, 1e-30f));
    }
  }
}
// pass A (dQ, lane = query row): tiles [t0, t0 + tiles) of the staged [tile][K (dual-use image: row reads for S^T, transposing reads
// for dQ^T) | V (row image)] against J 32-row query blocks; dq accumulates dQ^T without the 1/8 of the score scale
template <int J>
__device__ __forceinline__ void frame_pass_a(f32x16 (&dq)[J][2], const bf16x8 (&qf)[J][4], const bf16x8 (&dof)[J][4], const float (&lse)[J],
                                             const float (&delta)[J], const unsigned char* smem, int t0, int tiles, const FrameBwdLane& ln) {
  constexpr int TB = 64 * 128;
  const int kr0 = ln.kr0, vr0 = ln.vr0;
  const DualLane ktl = ln.kt;
#pragma unroll 1
  for (int t = t0; t < t0 + tiles; ++t) {
    const unsigned char* Kt = smem + t * 2 * TB;
    const unsigned char* Vt = Kt + TB;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      bf16x8 kf[4], vf[4], ktf[2][2];
      row_frag2(kf, vf, Kt, kr0, Vt, vr0, kt * 4096);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) ktf[s2][dt] = dual_read(Kt, ktl, kt * 32 + 16 * s2, dt);
#pragma unroll
      for (int j = 0; j < J; ++j) {
        f32x16 s, dp;
#pragma unroll
        for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          s = mfma32(kf[ks], qf[j][ks], s);
          dp = mfma32(vf[ks], dof[j][ks], dp);
        }
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) s[rr] = __builtin_amdgcn_exp2f(s[rr] - lse[j]) * (dp[rr] - delta[j]);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const bf16x8 db = pack8(s, s2);
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) dq[j][dt] = mfma32(ktf[s2][dt], db, dq[j][dt]);
        }
      }
    }
  }
}
// pass B (dK / dV, lane = key row) of an 8-wave workgroup: K / V row fragments of this wave's 32 keys from region A (tile wave / 2,
// rows (wave & 1) * 32 + r), Q | dO (both in the dual-use image) of tiles [t0, t0 + tiles) from region B, the rows' lse / delta
// from LDS; dk accumulates against q' = c q, with the 1/8 of the score scale applied
// (dK / dV come back BY VALUE: handed back through reference parameters, hipcc fused 18 more products of the raw-qkv kernel's adjoint
// stores into their sums than in the kernel that carried this body itself -- other bits in dqkv; scratch/attn_shared_parts_asm.py
// compares the floating-point opcode counts of every kernel for this reason)
struct FrameDkv { f32x16 dk[2], dv[2]; };
__device__ __forceinline__ FrameDkv frame_pass_b(const unsigned char* regA, const unsigned char* regB, const float* lse_lds,
                                             const float* del_lds, int wave, int t0, int tiles, const FrameBwdLane& ln) {
  constexpr int TB = 64 * 128;
  const int kr0 = ln.kr0, vr0 = ln.vr0, h = ln.h;
  const DualLane ktl = ln.kt;
  const unsigned char* Kown = regA + (wave >> 1) * 2 * TB + (wave & 1) * 4096;
  const unsigned char* Vown = Kown + TB;
  bf16x8 kf[4], vf[4];
  row_frag2(kf, vf, Kown, kr0, Vown, vr0, 0);
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) { dk[0][i] = 0.f; dk[1][i] = 0.f; dv[0][i] = 0.f; dv[1][i] = 0.f; }
#pragma unroll 1
  for (int t = t0; t < t0 + tiles; ++t) {
    const unsigned char* Qt = regB + t * 2 * TB;
    const unsigned char* dOt = Qt + TB;
#pragma unroll 1
    for (int qt = 0; qt < 2; ++qt) {
      bf16x8 qa[4], da[4], dotf[2][2], qtf[2][2];
      row_frag2(qa, da, Qt, kr0, dOt, kr0, qt * 4096);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dotf[s2][dt] = dual_read(dOt, ktl, qt * 32 + 16 * s2, dt);
          qtf[s2][dt] = dual_read(Qt, ktl, qt * 32 + 16 * s2, dt);
        }
      f32x16 s, dp, pv;
#pragma unroll
      for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s = mfma32(qa[ks], kf[ks], s);                   // S[q][key]
        dp = mfma32(da[ks], vf[ks], dp);                 // dP[q][key]
      }
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int qb4 = t * 64 + qt * 32 + 8 * g4 + 4 * h;
        const float4 ls = *(const float4*)(lse_lds + qb4), de = *(const float4*)(del_lds + qb4);
        const float lsv[4] = {ls.x, ls.y, ls.z, ls.w}, dev[4] = {de.x, de.y, de.z, de.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int rr = 4 * g4 + k;
          const float p = __builtin_amdgcn_exp2f(s[rr] - lsv[k]);
          pv[rr] = p;
          s[rr] = p * (dp[rr] - dev[k]) * 0.125f;
        }
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 pb = pack8(pv, s2);
        const bf16x8 db = pack8(s, s2);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dv[dt] = mfma32(dotf[s2][dt], pb, dv[dt]);
          dk[dt] = mfma32(qtf[s2][dt], db, dk[dt]);
        }
      }
    }
  }
  return FrameDkv{{dk[0], dk[1]}, {dv[0], dv[1]}};
}
// the backward kernels' own rows (lane = row, this lane's half of the 64 channels): Q and dO fragments, delta = dO . O; the three loads
// of a k-step share one branch and the products are summed inside the k-step loop, as delta has always been summed
__device__ __forceinline__ void frame_bwd_own_rows(bf16x8 (&qf)[4], bf16x8 (&dof)[4], float& delta, const bf16* qp, const bf16* dop, const bf16* op,
                                                   bool in) {
  delta = 0.f;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    u32x4 v = u32x4{0u, 0u, 0u, 0u}, w = u32x4{0u, 0u, 0u, 0u}, o = u32x4{0u, 0u, 0u, 0u};
    if (in) {
      v = *(const u32x4*)(qp + ks * 16);
      w = *(const u32x4*)(dop + ks * 16);
      o = *(const u32x4*)(op + ks * 16);
    }
    qf[ks] = __builtin_bit_cast(bf16x8, v);
    dof[ks] = __builtin_bit_cast(bf16x8, w);
    const bf16x8 ofr = __builtin_bit_cast(bf16x8, o);
#pragma unroll
    for (int e = 0; e < 8; ++e) delta += bf2f(dof[ks][e]) * bf2f(ofr[e]);
  }
  delta += __shfl_xor(delta, 32);
}

// J = 32-row query blocks per wave: 2 = a workgroup per 256 tokens (training); 1 = a workgroup per 128 tokens of a 256-token frame
// (round 6: one frame per sequence in the cached sampler is heads workgroups -- two query halves per frame put the launch on twice the
// CUs with half the MFMA / softmax chain each; K | V of the frame are staged by both)
template <int J>
__global__ __launch_bounds__(256, 2) void frame_attn_fwd_kernel(const FrameAttnDev d) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int TB = 64 * 128;
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * 2 * TB];     // [tile][K | V]
  const OnirisAttnArgs& a = d.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, C = a.C, P = a.Lq;
  const long long tok0 = (long long)(blockIdx.x / (2 / J)) * 256;            // the 256-token block whose K | V are staged
  const int qoff = (J == 2) ? 0 : (int)(blockIdx.x & 1) * 128;               // ... and this workgroup's query rows inside it
  const unsigned lds0 = (unsigned)(size_t)(lds_void_t*)smem;
  // Q fragments first (ordinary loads), consumed before any LDS-DMA is in flight
  const long long row0 = tok0 + qoff + wave * (32 * J) + r;                  // this lane's query rows: row0 + 32 j
  bf16x8 qf[J][4];
#pragma unroll
  for (int j = 0; j < J; ++j) own_row(qf[j], (const bf16*)a.q + (size_t)(row0 + j * 32) * C + head * 64 + h * 8, row0 + j * 32 < d.ntok);
  frame_burst<IMG_ROW, IMG_TR, 256>((const bf16*)a.k, (const bf16*)a.v, tok0, d.ntok, C, C, head, lds0, tid);
  f32x16 o[J][2];
  float l2[J][2];
#pragma unroll
  for (int j = 0; j < J; ++j) {
#pragma unroll
    for (int i = 0; i < 16; ++i) { o[j][0][i] = 0.f; o[j][1][i] = 0.f; }
    l2[j][0] = 0.f; l2[j][1] = 0.f;
  }
  const FrameFwdLane ln = frame_fwd_lane(lane);
  dma_wait();
  __syncthreads();
  const int t0 = ((qoff + wave * (32 * J)) / P) * d.tiles;  // first key tile of this wave's frame inside the super-block
  frame_fwd_tiles<J>(o, l2, qf, smem, t0, d.tiles, ln);
  frame_fwd_store<J>(o, l2, row0, d.ntok, (bf16*)a.out, a.lse, C, P, a.heads, head, h);
#endif
}

// dQ: the forward's structure (lane = query row); K in the dual-use image (row reads for S^T, transposing reads for dQ^T), V row-read
__global__ __launch_bounds__(256, 2) void frame_attn_dq_kernel(const FrameAttnDev d) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int TB = 64 * 128;
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * 2 * TB];     // [tile][K | V]
  const OnirisAttnArgs& a = d.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, C = a.C, P = a.Lq;
  const long long tok0 = (long long)blockIdx.x * 256;
  const unsigned lds0 = (unsigned)(size_t)(lds_void_t*)smem;
  bf16x8 qf[2][4], dof[2][4];
  float lse[2] = {0.f, 0.f}, delta[2] = {0.f, 0.f};
  const long long row0 = tok0 + wave * 64 + r;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const long long qrow = row0 + j * 32;
    const bool in = qrow < d.ntok;
    own_row(qf[j], (const bf16*)a.q + (size_t)qrow * C + head * 64 + h * 8, in);
    own_row(dof[j], (const bf16*)a.dout + (size_t)qrow * C + head * 64 + h * 8, in);
    if (in) {
      const long long b = qrow / P;
      const size_t li = (size_t)(b * a.heads + head) * P + (qrow - b * P);
      lse[j] = a.lse[li];
      delta[j] = a.delta[li];
    }
  }
  frame_burst<IMG_DUAL, IMG_ROW, 256>((const bf16*)a.k, (const bf16*)a.v, tok0, d.ntok, C, C, head, lds0, tid);
  f32x16 dq[2][2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) { dq[j][0][i] = 0.f; dq[j][1][i] = 0.f; }
  const FrameBwdLane ln = frame_bwd_lane(lane);
  dma_wait();
  __syncthreads();
  frame_pass_a<2>(dq, qf, dof, lse, delta, smem, ((wave * 64) / P) * d.tiles, d.tiles, ln);
#pragma unroll
  for (int j = 0; j < 2; ++j)
    if (row0 + j * 32 < d.ntok) lane_row_store((bf16*)a.dq + (size_t)(row0 + j * 32) * C + head * 64, dq[j], 0.125f, h);
#endif
}

// ---- the whole backward of a super-block in ONE launch: delta, dQ, dK, dV ----------------------------------------------------
// Dense attention inside 256-token frames is HBM-bound (4 * 64 * P FLOP per 4 * 128 B token row of q | k | v | out: 128 FLOP/B at
// P = 256, a third of the ridge), so the lever is bytes: attn_delta (reads dO, O) + dQ (reads q, k, v, dO) + dK/dV (reads q, k, v,
// dO) moved 13 tensor passes; here q, k, v, O, dO are read ONCE and dq, dk, dv written: 8 passes.
// 8 waves = 8 x 32 rows.  Pass A (lane = query): this wave's Q / dO / O rows from global (delta = dO . O in registers, lse | delta
// parked in LDS for pass B), K (dual-use image) | V (row image) of the super-block from LDS region A -> dQ.  Pass B (lane = key):
// K / V row fragments of this wave's 32 keys from region A, Q | dO (dual-use images) from region B -> dK, dV.  Both regions are
// requested up front; pass A starts as soon as region A has landed (counted vmcnt: region B's 8 copies stay in flight under it).
__global__ __launch_bounds__(512, 2) void frame_attn_bwd_kernel(const FrameAttnDev d) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int TB = 64 * 128, REG = 4 * 2 * TB;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * REG + 2048];     // A: [tile][K | V], B: [tile][Q | dO], lse[256] | delta[256]
  const OnirisAttnArgs& a = d.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, C = a.C, P = a.Lq;
  const long long tok0 = (long long)blockIdx.x * 256;
  const unsigned lds0 = (unsigned)(size_t)(lds_void_t*)smem;
  float* lse_lds = (float*)(smem + 2 * REG);
  float* del_lds = lse_lds + 256;
  const long long row = tok0 + wave * 32 + r;                // this lane's query row (pass A) = key row (pass B)
  const bool in = row < d.ntok;
  // ---- this wave's Q / dO / O rows, lse; delta
  bf16x8 qf[1][4], dof[1][4];
  float lse[1] = {0.f}, delta[1];
  {
    const size_t base = (size_t)row * C + head * 64 + h * 8;
    frame_bwd_own_rows(qf[0], dof[0], delta[0], (const bf16*)a.q + base, (const bf16*)a.dout + base, (const bf16*)a.out + base, in);
    if (in) {
      const long long b = row / P;
      lse[0] = a.lse[(size_t)(b * a.heads + head) * P + (row - b * P)];
    }
    if (h == 0) { lse_lds[wave * 32 + r] = lse[0]; del_lds[wave * 32 + r] = delta[0]; }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) asm volatile("" ::"v"(qf[0][ks]));      // every ordinary load consumed before an LDS-DMA is in flight
  }
  frame_burst<IMG_DUAL, IMG_ROW, 512>((const bf16*)a.k, (const bf16*)a.v, tok0, d.ntok, C, C, head, lds0, tid);
  frame_burst<IMG_DUAL, IMG_DUAL, 512>((const bf16*)a.q, (const bf16*)a.dout, tok0, d.ntok, C, C, head, lds0 + REG, tid);
  const int t0 = ((wave * 32) / P) * d.tiles;                // first tile of this wave's frame inside the super-block
  const FrameBwdLane ln = frame_bwd_lane(lane);
  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");           // region A (the first 8 copies of this wave) has landed
  __syncthreads();
  // ---- pass A: dQ
  {
    f32x16 dq[1][2];
#pragma unroll
    for (int i = 0; i < 16; ++i) { dq[0][0][i] = 0.f; dq[0][1][i] = 0.f; }
    frame_pass_a<1>(dq, qf, dof, lse, delta, smem, t0, d.tiles, ln);
    if (in) lane_row_store((bf16*)a.dq + (size_t)row * C + head * 64, dq[0], 0.125f, h);
  }
  dma_wait();                                                // region B has landed (and this wave's dQ stores are out)
  __syncthreads();
  // ---- pass B: dK, dV
  {
    const FrameDkv g = frame_pass_b(smem, smem + REG, lse_lds, del_lds, wave, t0, d.tiles, ln);
    if (in) {
      lane_row_store((bf16*)a.dk + (size_t)row * C + head * 64, g.dk, 1.f / SCALE_LOG2, h);
      lane_row_store((bf16*)a.dv + (size_t)row * C + head * 64, g.dv, 1.f, h);
    }
  }
#endif
}

// ---- the same two kernels on the RAW attn_qkv output -----------------------------------------------------------------------------
// FrameAttention normalises every 64-channel head vector of q, k and v (attention_modules.py:112: normalize(y, dim=-1)).  As a pass
// of its own (qkv_norm_kernel / qkv_norm_bwd_kernel) that moved 6 + 9 tensor rows per token around an attention kernel that moves
// 4 + 8: the normalisation was HALF of the layer's time (profiles/r06_ab_frame_attn.txt).  Here the kernels read qkv [tok][3C]
// (channel = s C + head 64 + c) directly: this wave's own rows are normalised in registers, the staged K / V (and Q) images are
// normalised IN LDS -- 8 lanes per 128-byte row, exactly the arithmetic of qkv_norm_kernel, values rounded to bf16 where the
// two-pass form rounded them -- and the backward's epilogues apply the adjoint of the normalisation (qkv_norm_bwd_kernel's formula)
// to dq, dk, dv while they are fp32 accumulators and write dqkv.
// one [4 tiles][64 rows][128 B] image inside a region (tile stride 2 TB): x <- x * scale / (eps + |x| / 8) per row
// sum over the 8 consecutive lanes that share a row (lanes 8k .. 8k+7), every lane gets the total: two quad permutes and a
// half-row mirror on the DPP path (full-rate VALU) -- __shfl_xor is a ds_bpermute round trip through LDS, three of them per pass
// made this phase the longest of the forward (profiles/r06_frame_attn_stamps.txt: 11.6 K of 40 K cycles)
__device__ __forceinline__ float row8_sum(float v) {
  int x = __builtin_bit_cast(int, v);
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true));      // quad_perm [1,0,3,2]
  x = __builtin_bit_cast(int, v);
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true));      // quad_perm [2,3,0,1]
  x = __builtin_bit_cast(int, v);
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true));     // row_half_mirror: quad 0 <-> quad 1
  return v;
}

template <int NT>
__device__ __forceinline__ void frame_lds_norm(unsigned char* img, float scale, int tid) {
  constexpr int TB = 64 * 128;
#pragma unroll
  for (int pass = 0; pass < 2048 / NT; ++pass) {
    const int e = pass * NT + tid, R = e >> 3, p = e & 7;
    bf16x8* at = (bf16x8*)(img + (R >> 6) * 2 * TB + (R & 63) * 128 + p * 16);
    const bf16x8 x = *at;
    float f[8], ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) { f[i] = bf2f(x[i]); ss += f[i] * f[i]; }
    ss = row8_sum(ss);
    const float inv = scale * __builtin_amdgcn_rcpf(1e-4f + __builtin_amdgcn_sqrtf(ss) * 0.125f);
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = f2bf(f[i] * inv);
    *at = o;
  }
}

// this lane's half (channels ks * 16 + h * 8 + 0..7, ks = 0..3) of a raw 64-channel row -> normalised fragments
__device__ __forceinline__ void frame_row_norm(bf16x8 (&f)[4], float scale) {
  float ss = 0.f;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int e = 0; e < 8; ++e) ss += bf2f(f[ks][e]) * bf2f(f[ks][e]);
  ss += __shfl_xor(ss, 32);
  const float inv = scale * __builtin_amdgcn_rcpf(1e-4f + __builtin_amdgcn_sqrtf(ss) * 0.125f);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int e = 0; e < 8; ++e) f[ks][e] = f2bf(bf2f(f[ks][e]) * inv);
}

struct FrameQkvDev {
  const bf16* qkv; bf16* out; float* lse; const bf16* dout; bf16* dqkv;
  long long ntok;
  int P, heads, C, tiles;
};
#ifdef FRAME_STAMP          // diagnostic build (make variant VSRC=attention VNAME=fstamp): 8 x s_memrealtime per workgroup into `lse + off`
#define FSTAMP(i) do { if (tid == 0) fst[i] = __builtin_readcyclecounter(); } while (0)
#else
#define FSTAMP(i) do { } while (0)
#endif

__global__ __launch_bounds__(256, 2) void frame_attn_qkv_fwd_kernel(const FrameQkvDev d) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int TB = 64 * 128;
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * 2 * TB];     // [tile][K | V]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, C = d.C, C3 = 3 * d.C, P = d.P;
  const long long tok0 = (long long)blockIdx.x * 256;
  const unsigned lds0 = (unsigned)(size_t)(lds_void_t*)smem;
#ifdef FRAME_STAMP
  long long* fst = (long long*)d.dqkv + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 8;
#endif
  FSTAMP(0);
  // K | V of the super-block are requested first; this wave's Q rows are loaded and normalised under the copy (the compiler's
  // wait for these ordinary loads also covers the older LDS-DMA copies: both are needed before the barrier anyway)
  frame_burst<IMG_ROW, IMG_TR, 256>(d.qkv + C, d.qkv + 2 * C, tok0, d.ntok, C3, C3, head, lds0, tid);
  FSTAMP(1);
  const long long row0 = tok0 + wave * 64 + r;                         // this lane's query rows: row0 + 32 j
  bf16x8 qf[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {            // (not own_row: with it hipcc fuses 54 more products of frame_row_norm's sums of squares below)
    const long long qrow = row0 + j * 32;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      u32x4 v = u32x4{0u, 0u, 0u, 0u};
      if (qrow < d.ntok) v = *(const u32x4*)(d.qkv + head * 64 + (size_t)qrow * C3 + ks * 16 + h * 8);
      qf[j][ks] = __builtin_bit_cast(bf16x8, v);
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) frame_row_norm(qf[j], SCALE_LOG2);      // q' = log2(e) / 8 * normalised q (one rounding, as qkv_norm_kernel)
  FSTAMP(2);
  f32x16 o[2][2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) { o[j][0][i] = 0.f; o[j][1][i] = 0.f; }
  float l2[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  const FrameFwdLane ln = frame_fwd_lane(lane);
  dma_wait();
  __syncthreads();
  FSTAMP(3);
  frame_lds_norm<256>(smem, 1.f, tid);                 // K
  frame_lds_norm<256>(smem + TB, 1.f, tid);            // V
  __syncthreads();
  FSTAMP(4);
  frame_fwd_tiles<2>(o, l2, qf, smem, ((wave * 64) / P) * d.tiles, d.tiles, ln);
  FSTAMP(5);
  frame_fwd_store<2>(o, l2, row0, d.ntok, d.out, d.lse, C, P, d.heads, head, h);
  FSTAMP(6);
#endif
}

__device__ __forceinline__ void qkv_norm_adjoint(float ss, float dot, float& k1, float& k2);     // (attention_qkv.h)

// adjoint of x -> x / (eps + |x| / 8) on this lane's half of a row held as fp32 accumulators g[dt][4 g4 + k] <-> channel
// dt * 32 + 8 g4 + 4 h + k (qkv_norm_bwd_kernel: o = g k1 - x k2), written to `dst` (the row's 64-channel slot of dqkv); x from `src`
__device__ __forceinline__ void frame_norm_adjoint_store(const f32x16 (&g)[2], float gscale, const bf16* src, bf16* dst, int h) {
  float x[2][16], ss = 0.f, dot = 0.f;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const bf16x4 v = *(const bf16x4*)(src + lane_row_ch(dt, g4, h));
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float f = bf2f(v[k]);
        x[dt][4 * g4 + k] = f;
        ss += f * f;
        dot += f * (g[dt][4 * g4 + k] * gscale);
      }
    }
  ss += __shfl_xor(ss, 32);
  dot += __shfl_xor(dot, 32);
  float k1, k2;
  qkv_norm_adjoint(ss, dot, k1, k2);
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      bf16x4 ov;
#pragma unroll
      for (int k = 0; k < 4; ++k) ov[k] = f2bf(g[dt][4 * g4 + k] * gscale * k1 - x[dt][4 * g4 + k] * k2);
      *(bf16x4*)(dst + lane_row_ch(dt, g4, h)) = ov;
    }
}

__global__ __launch_bounds__(512, 2) void frame_attn_qkv_bwd_kernel(const FrameQkvDev d) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int TB = 64 * 128, REG = 4 * 2 * TB;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * REG + 2048];     // A: [tile][K | V], B: [tile][Q | dO], lse[256] | delta[256]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, C = d.C, C3 = 3 * d.C, P = d.P;
  const long long tok0 = (long long)blockIdx.x * 256;
  const unsigned lds0 = (unsigned)(size_t)(lds_void_t*)smem;
  float* lse_lds = (float*)(smem + 2 * REG);
  float* del_lds = lse_lds + 256;
  const long long row = tok0 + wave * 32 + r;                // this lane's query row (pass A) = key row (pass B)
  const bool in = row < d.ntok;
  frame_burst<IMG_DUAL, IMG_ROW, 512>(d.qkv + C, d.qkv + 2 * C, tok0, d.ntok, C3, C3, head, lds0, tid);      // region A; the own rows load under it
  bf16x8 qf[1][4], dof[1][4];
  float lse[1] = {0.f}, delta[1];
  {
    frame_bwd_own_rows(qf[0], dof[0], delta[0], d.qkv + (size_t)row * C3 + head * 64 + h * 8, d.dout + (size_t)row * C + head * 64 + h * 8,
                       d.out + (size_t)row * C + head * 64 + h * 8, in);
    frame_row_norm(qf[0], SCALE_LOG2);
    if (in) {
      const long long b = row / P;
      lse[0] = d.lse[(size_t)(b * d.heads + head) * P + (row - b * P)];
    }
    if (h == 0) { lse_lds[wave * 32 + r] = lse[0]; del_lds[wave * 32 + r] = delta[0]; }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) asm volatile("" ::"v"(qf[0][ks]));      // every ordinary load consumed before region B is requested
  }
  frame_burst<IMG_DUAL, IMG_DUAL, 512>(d.qkv, d.dout, tok0, d.ntok, C3, C, head, lds0 + REG, tid);             // region B: lands under pass A
  const int t0 = ((wave * 32) / P) * d.tiles;
  const FrameBwdLane ln = frame_bwd_lane(lane);
  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");           // region A (the first 8 copies of this wave) has landed
  __syncthreads();
  frame_lds_norm<512>(smem, 1.f, tid);                        // K
  frame_lds_norm<512>(smem + TB, 1.f, tid);                   // V
  __syncthreads();
  // ---- pass A: dQ
  {
    f32x16 dq[1][2];
#pragma unroll
    for (int i = 0; i < 16; ++i) { dq[0][0][i] = 0.f; dq[0][1][i] = 0.f; }
    frame_pass_a<1>(dq, qf, dof, lse, delta, smem, t0, d.tiles, ln);
    if (in) frame_norm_adjoint_store(dq[0], 0.125f, d.qkv + (size_t)row * C3 + head * 64, d.dqkv + (size_t)row * C3 + head * 64, h);
  }
  dma_wait();                                                // region B has landed (and this wave's dq stores are out)
  __syncthreads();
  frame_lds_norm<512>(smem + REG, SCALE_LOG2, tid);           // Q (the image pass B multiplies: q' as in the forward)
  __syncthreads();
  // ---- pass B: dK, dV
  {
    const FrameDkv g = frame_pass_b(smem, smem + REG, lse_lds, del_lds, wave, t0, d.tiles, ln);
    if (in) {
      frame_norm_adjoint_store(g.dk, 1.f / SCALE_LOG2, d.qkv + (size_t)row * C3 + C + head * 64, d.dqkv + (size_t)row * C3 + C + head * 64, h);
      frame_norm_adjoint_store(g.dv, 1.f, d.qkv + (size_t)row * C3 + 2 * C + head * 64, d.dqkv + (size_t)row * C3 + 2 * C + head * 64, h);
    }
  }
#endif
}

// the frame kernels serve: dense (mask_mode 0), no table, no KV ring strides, no split-KV, Lq == Lk == P in {64, 128, 256}
static inline bool frame_attn_ok(const OnirisAttnArgs& a) {
  return !(a.frame_kernel & 1) && a.mask_mode == 0 && !a.kv_num && !a.sched && a.kv_splits <= 1 && a.k_bstride == 0 && a.v_bstride == 0 &&
         a.Lq == a.Lk && (a.Lq == 64 || a.Lq == 128 || a.Lq == 256);
}
