// The attention prologue: nine small kernels that normalise q | k | v per 64-channel head (x / (eps + |x| / 8)), rotate q and k
// (RoPe.py) and place k | v dense or in the KV ring, with the adjoints of the training path -- and, in front of them, the parts
// they are made of.  Included by attention.hip where the kernels stood (the same translation unit, the same compiler flags); the
// entry points stay in attention.hip.
//
// As in attention_parts.h / conv_parts.h every floating-point operation is written ONCE, in the order the result bits depend on:
// the sampler needs the one-launch path (qkv_eval_kernel / qkv_eval_few_kernel), the two-launch path (conv, then
// qkv_norm_rope_eval_kernel) and the three-launch path (conv, qkv_norm_kernel, rope_kernel) to round identically, and the
// adjoints to match the frame kernels'.  Two lane layouts:
//   8-lane   8 lanes x 8 channels cover a head vector (256 threads = 32 vectors per workgroup); the rotation partner c ^ 32 of a
//            channel is the same register of lane ^ 4;
//   MFMA     one token per lane pair, the accumulators of D[channel][token]: register i of acc[0] / acc[1] is channel
//            8 (i / 4) + 4 h + i % 4 of the first / second half of the head, so the rotation partner is the other accumulator.
#pragma once

// ---- 8-lane layout ---------------------------------------------------------------------------------------------------
// thread -> (vector, part = which 8 channels of it); false: beyond the last vector (nvec * 8 is a multiple of 64 wherever a
// kernel shuffles afterwards, so whole waves leave together)
__device__ __forceinline__ bool lane8_vec(long long& vec, int& part, long long nvec) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  vec = gid >> 3;
  part = (int)(gid & 7);
  return vec < nvec;
}

// head vector `vi` = s * heads + hd of token `tok` in qkv [tok][3C] (channel = s * C + hd * 64 + c; s: 0 q, 1 k, 2 v)
struct QkvVec {
  long long tok;
  int vi, s, hd, part;
  __device__ __forceinline__ long long in(int C) const { return tok * 3 * C + (size_t)vi * 64 + part * 8; }      // this lane's 8 channels in qkv / dqkv
  __device__ __forceinline__ long long out(int C) const { return tok * C + hd * 64 + part * 8; }                 // ... in a dense q | k | v [tok][C]
};
__device__ __forceinline__ bool qkv_vec(QkvVec& t, long long nvec, int C) {
  long long vec;
  if (!lane8_vec(vec, t.part, nvec)) return false;
  const int hpt = 3 * C / 64;                       // vectors per token
  t.tok = vec / hpt;
  t.vi = (int)(vec % hpt);
  t.s = t.vi / (C / 64);
  t.hd = t.vi % (C / 64);
  return true;
}
__device__ __forceinline__ const bf16* qkv_pick(int s, const bf16* q, const bf16* k, const bf16* v) { return (s == 0) ? q : (s == 1) ? k : v; }
__device__ __forceinline__ bf16* qkv_pick(int s, bf16* q, bf16* k, bf16* v) { return (s == 0) ? q : (s == 1) ? k : v; }

// sum over the 8 lanes of a head vector
__device__ __forceinline__ float row8_add(float v) {
  v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
  return v;
}
// 8 channels at p, widened into f -> the head vector's sum of squares
__device__ __forceinline__ float qkv_row8_sq(const bf16* p, float (&f)[8]) {
  const bf16x8 x = *(const bf16x8*)p;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) { f[i] = bf2f(x[i]); ss += f[i] * f[i]; }
  return row8_add(ss);
}
__device__ __forceinline__ void store8(bf16* p, const float (&f)[8]) {
  bf16x8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = f2bf(f[i]);
  *(bf16x8*)p = o;
}

// eps + |x| / 8 of a head vector of norm n
__device__ __forceinline__ float qkv_den(float n) { return 1e-4f + n * 0.125f; }
// 1 / (eps + |x| / 8) from the sum of squares of a head vector.  q (s == 0) leaves with the softmax scale folded in (one
// rounding): q' = log2(e)/8 * normalised q, so that every attention kernel gets its log2-domain scores straight out of the MFMA
// (exp2(q'.k - lse), no multiply per score element)
__device__ __forceinline__ float qkv_inv(float ss, int s) { return ((s == 0) ? SCALE_LOG2 : 1.f) / qkv_den(sqrtf(ss)); }

// adjoint of x -> x / (eps + |x| / 8): dx = g k1 - x k2 (ss = x.x, dot = x.g over the head vector)
__device__ __forceinline__ void qkv_norm_adjoint(float ss, float dot, float& k1, float& k2) {
  const float n = sqrtf(ss), sden = qkv_den(n);
  k1 = 1.f / sden;
  k2 = (n > 0.f) ? dot * 0.125f / (sden * sden * n) : 0.f;
}
// ... of this lane's 8 channels (ss, dot: this lane's part of the sums), dx to p.  The kernels sum x x and x g in ONE loop with the
// widening: hipcc packs the squares of a loop of their own into v_pk_mul_f32 and then fuses none of them into the sum -- another
// rounding
__device__ __forceinline__ void qkv_norm_adjoint_store(bf16* p, const float (&f)[8], const float (&gg)[8], float ss, float dot) {
  float k1, k2, o[8];
  qkv_norm_adjoint(row8_add(ss), row8_add(dot), k1, k2);
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = gg[i] * k1 - f[i] * k2;
  store8(p, o);
}

// the rotary tables [pos][64] fp32 (cos, sin, scale; each duplicated over the two halves like RoPe.py:21-32): 8 channels of a row
// as two 16-byte loads (element-wise 4-byte loads made qkv_norm_rope_kernel VMEM-issue bound: 24 table loads per 16 bytes of
// output, 1.7 TB/s)
struct RopeTab8 { float cs[8], sn[8], sc[8]; };
struct RopeTabPtr { const float *cs, *sn, *sc; };   // the same 8 channels read where they are used
__device__ __forceinline__ void qkv_tab8(const float* t, size_t tb, float (&out)[8]) {
  *(float4*)&out[0] = *(const float4*)(t + tb); *(float4*)&out[4] = *(const float4*)(t + tb + 4);
}
__device__ __forceinline__ void qkv_tabs8(RopeTab8& t, const float* cos_t, const float* sin_t, const float* scale_t, size_t tb) {
  qkv_tab8(cos_t, tb, t.cs); qkv_tab8(sin_t, tb, t.sn); qkv_tab8(scale_t, tb, t.sc);
}

// rotate_half is [-x2, x1]: the sign of the partner's term for a channel of the first (`low`) or second half; the adjoint takes
// the opposite sign
__device__ __forceinline__ float rope_sign(bool low) { return low ? -1.f : 1.f; }
// one channel of R a (a1 = the partner channel, sg = rope_sign), then the learned scale: q * scale, k / scale
__device__ __forceinline__ float rope_rotate(float a0, float a1, float sg, float cs, float sn, float scl, bool mul) {
  const float val = a0 * cs + sg * a1 * sn;
  return mul ? val * scl : val / scl;
}
// 8-lane layout, forward: channel i of this lane's normalised u against the same register of lane ^ 4 (every lane of the 8-lane
// group takes part in the shuffle: call it outside divergent code); v (s == 2) passes
template <class Tab>
__device__ __forceinline__ float qkv_rot8(float u, int s, float sg, const Tab& t, int i) {
  const float up = __shfl_xor(u, 4);
  return (s != 2) ? rope_rotate(u, up, sg, t.cs[i], t.sn[i], t.sc[i], s == 0) : u;
}
// ... adjoint: R^T g = g cos - rot(g sin), and the scale vector is equal in both halves, so it commutes with the rotation
__device__ __forceinline__ float qkv_rot8_adjoint(float gv, int s, float sg, const RopeTab8& t, int i) {
  if (s != 2) gv = (s == 0) ? gv * t.sc[i] : gv / t.sc[i];
  const float gs = (s != 2) ? gv * t.sn[i] : 0.f;
  const float gp = __shfl_xor(gs, 4);               // (g sin) of the partner channel
  return (s != 2) ? gv * t.cs[i] + sg * gp : gv;
}

// KV ring: a sequence owns kv_bstride elements and takes kv_tpb tokens per launch; token tok = b * kv_tpb + r lands in row
// kv_off + r of sequence b (one sequence: tok < kv_tpb, no 64-bit division on the way to the stores).  -> element of the row
__device__ __forceinline__ long long qkv_ring_row(long long tok, long long kv_tpb, long long kv_bstride, long long kv_off, int C) {
  const long long sq = (tok < kv_tpb) ? 0 : tok / kv_tpb;
  return sq * kv_bstride + (kv_off + tok - sq * kv_tpb) * C;
}

// ---- MFMA layout ------------------------------------------------------------------------------------------------------
// table row `pos` for the 2 x 16 channels of a lane (h = lane >> 5): cos, sin, scale (c, s, q) of the first half of the head (0) and the second (1)
struct RopeTabMfma { float c0[16], s0[16], c1[16], s1[16], q0[16], q1[16]; };
__device__ __forceinline__ void qkv_eval_tab(const float* t, size_t tb, int h, float (&lo)[16], float (&hi)[16]) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int c = 8 * g + 4 * h;
    const float4 a0 = *(const float4*)(t + tb + c), a1 = *(const float4*)(t + tb + c + 32);
    lo[4 * g] = a0.x; lo[4 * g + 1] = a0.y; lo[4 * g + 2] = a0.z; lo[4 * g + 3] = a0.w;
    hi[4 * g] = a1.x; hi[4 * g + 1] = a1.y; hi[4 * g + 2] = a1.z; hi[4 * g + 3] = a1.w;
  }
}
// (the values depend on the lane only: the kernels request them FIRST, so that their round trip runs under the tile loads instead
// of behind the MFMAs -- a launch is a latency chain, 129 of them make an evaluation)
__device__ __forceinline__ void qkv_eval_tabs(RopeTabMfma& t, const float* cos_t, const float* sin_t, const float* scale_t, int pos, int h) {
  const size_t tb = (size_t)pos * 64;
  qkv_eval_tab(cos_t, tb, h, t.c0, t.c1); qkv_eval_tab(sin_t, tb, h, t.s0, t.s1); qkv_eval_tab(scale_t, tb, h, t.q0, t.q1);
}

// where a launch of qkv_eval_kernel / qkv_eval_few_kernel writes: q [tok][C], k | v dense or in the ring, kr = the ring's rotated
// image; tokens >= split are the 2-D rows of a guided pair launch (oniris_qkv_eval_pair) -- normalised, un-rotated q | k | v, dense
// [token - split][C] in the side buffers (what the frame form of the launch writes)
struct QkvEvalOut {
  bf16 *q, *k, *v, *kr;
  long long kv_tpb, kv_bstride, kv_off, split;
  bf16 *q2, *k2, *v2;
  int C;
};

// The convolution result acc (head hd of slot s) of token `tok`, rounded to bf16 like the tensor the two-launch path stores in
// between, normalised, rotated where `rope` and stored.  Every lane of the wave calls it (the other half of the head is in
// lane ^ 32); lanes without a token (!valid) leave after the reduce.  As in qkv_norm_rope_eval_kernel the rotation sees the
// bf16-rounded normalised vector.
__device__ __forceinline__ void qkv_eval_epilogue(const f32x16 (&acc)[2], const RopeTabMfma& t, bool rope, long long tok, bool valid, int s,
                                                  int hd, int h, const QkvEvalOut& o) {
  float f[2][16], ss = 0.f;
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int i = 0; i < 16; ++i) { f[n][i] = bf2f(f2bf(acc[n][i])); ss += f[n][i] * f[n][i]; }
  ss += __shfl_xor(ss, 32);
  const float inv = qkv_inv(ss, s);
  if (!valid) return;
  const bool side = tok >= o.split;
  bf16* const qo = side ? o.q2 : o.q;
  bf16* const ko = side ? o.k2 : o.k;
  bf16* const vo = side ? o.v2 : o.v;
  const bool rot_on = rope && !side;
  const long long dense = (side ? tok - o.split : tok) * o.C + hd * 64;
  long long ring = dense;
  if (o.kv_tpb > 0 && !side) ring = qkv_ring_row(tok, o.kv_tpb, o.kv_bstride, o.kv_off, o.C) + hd * 64;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    bf16x4 plain[2], rot[2];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int i = 4 * g + kk;                               // channel 8 g + 4 h + kk (first half) and + 32 (second half) of the head
      const float u0 = bf2f(f2bf(f[0][i] * inv)), u1 = bf2f(f2bf(f[1][i] * inv));
      plain[0][kk] = f2bf(u0); plain[1][kk] = f2bf(u1);
      float v0 = u0, v1 = u1;
      if (rot_on) {
        v0 = u0 * t.c0[i] - u1 * t.s0[i];                     // rotate_half: [-x2, x1]
        v1 = u1 * t.c1[i] + u0 * t.s1[i];
        const float s0 = t.q0[i], s1 = t.q1[i];
        v0 = (s == 0) ? v0 * s0 : v0 / s0;
        v1 = (s == 0) ? v1 * s1 : v1 / s1;
      }
      rot[0][kk] = f2bf(v0); rot[1][kk] = f2bf(v1);
    }
    const int co = 8 * g + 4 * h;
    if (s == 0) {
      *(bf16x4*)(qo + dense + co) = rot[0]; *(bf16x4*)(qo + dense + co + 32) = rot[1];
    } else if (s == 1) {
      *(bf16x4*)(ko + ring + co) = plain[0]; *(bf16x4*)(ko + ring + co + 32) = plain[1];
      if (o.kr && !side) { *(bf16x4*)(o.kr + ring + co) = rot[0]; *(bf16x4*)(o.kr + ring + co + 32) = rot[1]; }
    } else {
      *(bf16x4*)(vo + ring + co) = plain[0]; *(bf16x4*)(vo + ring + co + 32) = plain[1];
    }
  }
}

// ================================================================================================================
// the kernels

// qkv [tok][3C] -> q, k, v [tok][C], each 64-vector normalised.  kv_tpb > 0: k and v go to a KV ring (qkv_ring_row)
__global__ void qkv_norm_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ q, bf16* __restrict__ k,
                                bf16* __restrict__ v, long long nvec, int C, long long kv_tpb, long long kv_bstride,
                                long long kv_off) {
  QkvVec t;
  if (!qkv_vec(t, nvec, C)) return;
  float f[8];
  const float inv = qkv_inv(qkv_row8_sq(qkv + t.in(C), f), t.s);
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = f[i] * inv;
  long long row = t.tok * C;
  if (t.s != 0 && kv_tpb > 0) row = qkv_ring_row(t.tok, kv_tpb, kv_bstride, kv_off, C);
  store8(qkv_pick(t.s, q, k, v) + row + t.hd * 64 + t.part * 8, f);
}

__global__ void qkv_norm_bwd_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ dq,
                                    const bf16* __restrict__ dk, const bf16* __restrict__ dv,
                                    bf16* __restrict__ dqkv, long long nvec, int C) {
  QkvVec t;
  if (!qkv_vec(t, nvec, C)) return;
  const bf16x8 x = *(const bf16x8*)(qkv + t.in(C)), g = *(const bf16x8*)(qkv_pick(t.s, dq, dk, dv) + t.out(C));
  float f[8], gg[8], ss = 0.f, dot = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) { f[i] = bf2f(x[i]); gg[i] = bf2f(g[i]); ss += f[i] * f[i]; dot += f[i] * gg[i]; }
  qkv_norm_adjoint_store(dqkv + t.in(C), f, gg, ss, dot);
}

// qkv_norm_kernel + the rotary embedding of q and k in one pass (training: position = (token / P) mod pos_mod).  The normalised
// value is rotated in fp32: q, k are rounded to bf16 once (the two-kernel path rounds the normalised vector first).
//   q' = log2(e)/8 * (u cos + rot(u) sin) * scale,   k' = (u cos + rot(u) sin) / scale,   v' = u      (u = x/(eps+|x|/8))
__global__ void qkv_norm_rope_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ q, bf16* __restrict__ k,
                                     bf16* __restrict__ v, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                     const float* __restrict__ scale_t, long long nvec, int C, int P, int pos_mod) {
  QkvVec t;
  if (!qkv_vec(t, nvec, C)) return;
  float f[8];
  const float inv = qkv_inv(qkv_row8_sq(qkv + t.in(C), f), t.s);
  const float sg = rope_sign(t.part < 4);
  RopeTab8 tab;
  if (t.s != 2) qkv_tabs8(tab, cos_t, sin_t, scale_t, (size_t)((t.tok / P) % pos_mod) * 64 + t.part * 8);
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = qkv_rot8(f[i] * inv, t.s, sg, tab, i);
  store8(qkv_pick(t.s, q, k, v) + t.out(C), f);
}

// One NEW frame per sequence of the KV-cached sampler (attention_modules.py:51-70): normalisation of q, k, v and the rotary
// embedding of q and k at the frame's position `pos` (= n_keys - 1: tables row pos) in one pass.  Outputs: q rotated (with
// the softmax scale), k UN-rotated and v into the KV ring behind the committed frames (the cache keeps un-rotated keys:
// every later frame count re-rotates them, RoPe.py:55-57), k rotated into the ring's ROTATED image `kr`, whose committed
// frames were rotated once for this frame count (KVRing.rotate_committed) instead of once per UNet evaluation.
__global__ void qkv_norm_rope_eval_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ q, bf16* __restrict__ k,
                                          bf16* __restrict__ v, bf16* __restrict__ kr, const float* __restrict__ cos_t,
                                          const float* __restrict__ sin_t, const float* __restrict__ scale_t, long long nvec,
                                          int C, long long kv_tpb, long long kv_bstride, long long kv_off, int pos) {
  QkvVec t;
  if (!qkv_vec(t, nvec, C)) return;
  float f[8];
  const float inv = qkv_inv(qkv_row8_sq(qkv + t.in(C), f), t.s);
  const float sg = rope_sign(t.part < 4);
  const size_t tb = (size_t)pos * 64 + t.part * 8;
  const RopeTabPtr tab{cos_t + tb, sin_t + tb, scale_t + tb};
  bf16x8 plain, rot;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    // like the two-launch path (qkv_norm, then rope on its bf16 output) the rotation sees the bf16-rounded vector, so that
    // the rotated key of a frame is the same number whether it is rotated now or re-rotated from the ring later
    const float u = bf2f(f2bf(f[i] * inv));
    plain[i] = f2bf(u);
    rot[i] = f2bf(qkv_rot8(u, t.s, sg, tab, i));
  }
  const long long ring = qkv_ring_row(t.tok, kv_tpb, kv_bstride, kv_off, C) + t.hd * 64 + t.part * 8;
  if (t.s == 0) *(bf16x8*)(q + t.out(C)) = rot;
  else if (t.s == 1) { *(bf16x8*)(k + ring) = plain; *(bf16x8*)(kr + ring) = rot; }
  else *(bf16x8*)(v + ring) = plain;
}

// adjoint of qkv_norm_rope_kernel: dq (w.r.t. the UNSCALED rotated q, as the attention backward returns it), dk, dv -> dqkv
__global__ void qkv_norm_rope_bwd_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ dq,
                                         const bf16* __restrict__ dk, const bf16* __restrict__ dv, bf16* __restrict__ dqkv,
                                         const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                         const float* __restrict__ scale_t, long long nvec, int C, int P, int pos_mod) {
  QkvVec t;
  if (!qkv_vec(t, nvec, C)) return;
  const bf16x8 x = *(const bf16x8*)(qkv + t.in(C)), g = *(const bf16x8*)(qkv_pick(t.s, dq, dk, dv) + t.out(C));
  const float sg = rope_sign(t.part >= 4);          // adjoint of rotate_half: the other half's sign
  RopeTab8 tab;
  if (t.s != 2) qkv_tabs8(tab, cos_t, sin_t, scale_t, (size_t)((t.tok / P) % pos_mod) * 64 + t.part * 8);
  float f[8], gg[8], ss = 0.f, dot = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    f[i] = bf2f(x[i]);
    gg[i] = qkv_rot8_adjoint(bf2f(g[i]), t.s, sg, tab, i);
    ss += f[i] * f[i]; dot += f[i] * gg[i];
  }
  qkv_norm_adjoint_store(dqkv + t.in(C), f, gg, ss, dot);
}

// The sampler's attention input in ONE launch (31 evaluations per generated frame, every graph node costs ~5 us): the
// attn_qkv 1x1 convolution of the new frame(s) (MPConv, attention_modules.py:47), the per-head normalisation and -- when
// tables are given -- the rotary embedding at table row `pos`, written where qkv_norm_rope_eval_kernel / qkv_norm_kernel
// write: q [tok][C] (with the softmax scale), k / v dense or behind the committed frames of the KV ring, kr = the rotated
// key into the ring's rotated image.  One workgroup = 128 tokens x one (q|k|v, head) slice of 64 output channels; wave w
// owns tokens 32w..32w+31 (MFMA D[channel][token]: a lane holds 32 of the head's 64 channels of ONE token, lane ^ 32 the
// others); qkv_eval_epilogue does the rest.
template <int KC>
__global__ __launch_bounds__(256) void qkv_eval_kernel(const bf16* __restrict__ x, const bf16* __restrict__ w,
                                                       bf16* __restrict__ q, bf16* __restrict__ k, bf16* __restrict__ v,
                                                       bf16* __restrict__ kr, const float* __restrict__ cos_t,
                                                       const float* __restrict__ sin_t, const float* __restrict__ scale_t,
                                                       long long M, int C, int CinP, long long kv_tpb, long long kv_bstride,
                                                       long long kv_off, int pos, long long split, bf16* __restrict__ q2,
                                                       bf16* __restrict__ k2, bf16* __restrict__ v2) {
  // K is staged KC input channels at a time (the whole K for C <= 256: every load of the tile is in flight at once -- the
  // launch is pure latency, ~10 us with four 64-channel rounds of load / barrier / multiply, half of that in one round)
  constexpr int ROWB = KC * 2 + 16;                          // + 16 bytes: conflict-free 16-byte fragment reads
  constexpr int PCS = KC / 8;                                // 16-byte pieces per row
  __shared__ __attribute__((aligned(16))) unsigned char xs[128 * ROWB];
  __shared__ __attribute__((aligned(16))) unsigned char ws[64 * ROWB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const long long m0 = (long long)blockIdx.x * 128;
  // (slot and head from the grid: a division by a run-time value is ~40 instructions in front of the first address of a launch that
  // lasts 17 K cycles; round 6)
  const int hd = blockIdx.y, s = blockIdx.z, vi = s * (int)gridDim.y + hd;
  const bf16* wrow = w + (size_t)vi * 64 * CinP;
  const int mrows = (M - m0 < 128) ? (int)(M - m0) : 128;    // rows beyond M are never read back by a valid token
  f32x16 acc[2];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;
  const bool rope = cos_t != nullptr && s != 2;
  RopeTabMfma tab;
  if (rope) qkv_eval_tabs(tab, cos_t, sin_t, scale_t, pos, h);
  for (int c0 = 0; c0 < C; c0 += KC) {
    if (c0) __syncthreads();
#pragma unroll
    for (int i = 0; i < 64 * PCS / 256; ++i) {               // weight tile: 64 rows
      const int e = i * 256 + tid, row = e / PCS, pc = e % PCS;
      *(u32x4*)(ws + row * ROWB + pc * 16) = *(const u32x4*)(wrow + (size_t)row * CinP + c0 + pc * 8);
    }
#pragma unroll
    for (int i = 0; i < 128 * PCS / 256; ++i) {              // x tile: 128 rows
      const int e = i * 256 + tid, row = e / PCS, pc = e % PCS;
      if (row < mrows) *(u32x4*)(xs + row * ROWB + pc * 16) = *(const u32x4*)(x + (size_t)(m0 + row) * C + c0 + pc * 8);
    }
    __syncthreads();
    if (wave * 32 < mrows) {
#pragma unroll
      for (int ks = 0; ks < KC / 16; ++ks) {
        const bf16x8 xf = *(const bf16x8*)(xs + (wave * 32 + r) * ROWB + (ks * 2 + h) * 16);
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const bf16x8 wf = *(const bf16x8*)(ws + (n * 32 + r) * ROWB + (ks * 2 + h) * 16);
          acc[n] = mfma32(wf, xf, acc[n]);
        }
      }
    }
  }
  const long long tok = m0 + wave * 32 + r;
  qkv_eval_epilogue(acc, tab, rope, tok, tok < M, s, hd, h, QkvEvalOut{q, k, v, kr, kv_tpb, kv_bstride, kv_off, split, q2, k2, v2, C});
}

// qkv_eval_kernel for a FEW tiles (one frame per sequence in the cached sampler; round 6, after conv1x1_few.h): a workgroup owns 32 tokens x
// the 64 channels of one (slot, head) and its four waves split the K -- wave w takes the 64-channel rounds w, w + 4, ... with every operand
// loaded global -> registers in MFMA fragment layout (no LDS staging, no barrier in the K loop); the partial tiles meet in LDS once and
// wave 0 runs qkv_eval_epilogue (the conv result sums K in another order than qkv_eval_kernel's).
__global__ __launch_bounds__(256) void qkv_eval_few_kernel(const bf16* __restrict__ x, const bf16* __restrict__ w,
                                                           bf16* __restrict__ q, bf16* __restrict__ k, bf16* __restrict__ v,
                                                           bf16* __restrict__ kr, const float* __restrict__ cos_t,
                                                           const float* __restrict__ sin_t, const float* __restrict__ scale_t,
                                                           long long M, int C, int CinP, long long kv_tpb, long long kv_bstride,
                                                           long long kv_off, int pos, long long split, bf16* __restrict__ q2,
                                                           bf16* __restrict__ k2, bf16* __restrict__ v2) {
  __shared__ float red[3 * 2 * 16 * 64];           // waves 1..3 -> wave 0: [wave - 1][n-tile][accumulator register][lane]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 31, h = lane >> 5;
  const long long tok = (long long)blockIdx.x * 32 + r;
  const int hd = blockIdx.y, s = blockIdx.z, vi = s * (int)gridDim.y + hd;
  const bool tvalid = tok < M;
  const bf16* xrow = x + (size_t)(tvalid ? tok : 0) * C;
  const bf16* wrow0 = w + ((size_t)vi * 64 + r) * CinP;
  const bf16* wrow1 = wrow0 + (size_t)32 * CinP;
  const bool rope = cos_t != nullptr && s != 2;
  // (wave 0 runs the epilogue: its rotary-table values are requested first, like qkv_eval_kernel's)
  RopeTabMfma tab;
  if (rope && wave == 0) qkv_eval_tabs(tab, cos_t, sin_t, scale_t, pos, h);
  f32x16 acc[2];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;
  const int nround = C >> 6;
#pragma unroll 1
  for (int ch = wave; ch < nround; ch += 4) {
    const int c0 = ch * 64 + h * 8;
    u32x4 w0[4], w1[4], xv[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int c = c0 + ks * 16;
      w0[ks] = *(const u32x4*)(wrow0 + c);
      w1[ks] = *(const u32x4*)(wrow1 + c);
      xv[ks] = tvalid ? *(const u32x4*)(xrow + c) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bf16x8 xf = __builtin_bit_cast(bf16x8, xv[ks]);
      acc[0] = mfma32(__builtin_bit_cast(bf16x8, w0[ks]), xf, acc[0]);
      acc[1] = mfma32(__builtin_bit_cast(bf16x8, w1[ks]), xf, acc[1]);
    }
  }
  if (wave != 0) {
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int i = 0; i < 16; ++i) red[(((wave - 1) * 2 + n) * 16 + i) * 64 + lane] = acc[n][i];
  }
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int i = 0; i < 16; ++i)
      acc[n][i] = ((acc[n][i] + red[((0 * 2 + n) * 16 + i) * 64 + lane]) + red[((1 * 2 + n) * 16 + i) * 64 + lane]) +
                  red[((2 * 2 + n) * 16 + i) * 64 + lane];
  qkv_eval_epilogue(acc, tab, rope, tok, tvalid, s, hd, h, QkvEvalOut{q, k, v, kr, kv_tpb, kv_bstride, kv_off, split, q2, k2, v2, C});
}

// rotary embedding over the frame index (+ optional transposed copy); one workgroup = 64 tokens x 1 head.  mode 0: copy only,
// 1 / 2: q / k forward (* scale, / scale), 3 / 4: their adjoints
__global__ __launch_bounds__(256) void rope_kernel(const bf16* __restrict__ x, bf16* __restrict__ xr,
                                                   bf16* __restrict__ xt, const float* __restrict__ cos_t,
                                                   const float* __restrict__ sin_t, const float* __restrict__ scale_t,
                                                   int mode, int L, int P, int C, int heads, int pos_offset,
                                                   int pos_mod, long long x_bstride, long long xr_bstride) {
  __shared__ float tile[64][65];
  const int tid = threadIdx.x;
  const int tok0 = blockIdx.x * 64, head = blockIdx.y, b = blockIdx.z;
  const bf16* xg = x + (size_t)b * x_bstride + head * 64;
  {
    const int row = tid >> 2, part = tid & 3;       // 16 channels per thread
    const int tok = tok0 + row;
    bf16x8 v0, v1;
#pragma unroll
    for (int i = 0; i < 8; ++i) { v0[i] = f2bf(0.f); v1[i] = f2bf(0.f); }
    if (tok < L) {
      v0 = *(const bf16x8*)(xg + (size_t)tok * C + part * 16);
      v1 = *(const bf16x8*)(xg + (size_t)tok * C + part * 16 + 8);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) { tile[row][part * 16 + i] = bf2f(v0[i]); tile[row][part * 16 + 8 + i] = bf2f(v1[i]); }
  }
  __syncthreads();
  if (mode != 0) {
    const int row = tid >> 2, part = tid & 3;
    const int tok = tok0 + row;
    float out[16];
    if (tok < L) {
      const int pos = pos_offset + ((tok / P) % pos_mod);
      const float* cs = cos_t + (size_t)pos * 64;
      const float* sn = sin_t + (size_t)pos * 64;
      const float* sc = scale_t + (size_t)pos * 64;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = part * 16 + i;
        float sg = rope_sign(c < 32);
        if (mode >= 3) sg = -sg;                     // adjoint
        out[i] = rope_rotate(tile[row][c], tile[row][c ^ 32], sg, cs[c], sn[c], sc[c], mode == 1 || mode == 3);
      }
    }
    __syncthreads();
    if (tok < L) {
#pragma unroll
      for (int i = 0; i < 16; ++i) tile[row][part * 16 + i] = out[i];
    }
    __syncthreads();
  }
  if (xr) {
    const int row = tid >> 2, part = tid & 3;
    const int tok = tok0 + row;
    if (tok < L) {
      bf16x8 v0, v1;
#pragma unroll
      for (int i = 0; i < 8; ++i) { v0[i] = f2bf(tile[row][part * 16 + i]); v1[i] = f2bf(tile[row][part * 16 + 8 + i]); }
      bf16* dst = xr + (size_t)b * xr_bstride + head * 64 + (size_t)tok * C + part * 16;
      *(bf16x8*)dst = v0;
      *(bf16x8*)(dst + 8) = v1;
    }
  }
  if (xt) {
    const int ch = tid >> 2, part = tid & 3;        // 16 tokens per thread
    bf16* dst = xt + ((size_t)(b * heads + head) * 64 + ch) * L + tok0 + part * 16;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      if (tok0 + part * 16 + hh * 8 < L) {
        bf16x8 v;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = f2bf(tile[part * 16 + hh * 8 + i][ch]);
        *(bf16x8*)(dst + hh * 8) = v;
      }
    }
  }
}

// delta[b][h][tok] = sum_c dO * O
__global__ void attn_delta_kernel(const bf16* __restrict__ dout, const bf16* __restrict__ out, float* __restrict__ delta,
                                  const float* __restrict__ lse, float* __restrict__ neg, long long nvec, int L, int C,
                                  int heads) {
  long long vec;
  int part;
  if (!lane8_vec(vec, part, nvec)) return;
  const long long tokg = vec / heads;                // b*L + tok
  const int hd = (int)(vec % heads);
  const bf16x8 a = *(const bf16x8*)(dout + tokg * C + hd * 64 + part * 8);
  const bf16x8 o = *(const bf16x8*)(out + tokg * C + hd * 64 + part * 8);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += bf2f(a[i]) * bf2f(o[i]);
  s = row8_add(s);
  if (part == 0) {
    const long long bb = tokg / L, tok = tokg % L;
    const long long at = (bb * heads + hd) * L + tok;
    delta[at] = s;
    if (neg) {                                     // row constants of the persistent dK/dV kernel: [0] = -lse, [1] = -delta
      neg[at] = -lse[at];
      neg[nvec + at] = -s;
    }
  }
}
