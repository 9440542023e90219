// VAE training losses (reference: edm2/utils.py GaussianLoss :209-210, F.l1_loss / F.mse_loss, edm2/vae/utils.py
// worst_k_percent_loss :54-68), fp32 throughout.  include/oniris.h: oniris_vae_loss_*.
//   oniris_vae_loss_fwd          one pass over mean | logvar | target -> per-workgroup partials [P][3] of the Gaussian, L1 and MSE
//                                means (already times 1 / n; oniris_disc_part_sum adds them up)
//   oniris_vae_loss_bwd          one pass: d mean, d logvar, d target from the three upstream cotangents (device scalars)
//   oniris_vae_loss_topk_keys    e = (recon - target)^2 once, contiguous, plus the histogram of the top 11 key bits
//   oniris_vae_loss_topk_count   histogram of the next 10 bits over the elements that match the prefix fixed so far; the last
//                                pass also sums e over everything above the prefix
//   oniris_vae_loss_topk_select  one workgroup: scans a histogram from the top bin and fixes the next digit; after the last digit
//                                it writes the loss and the saved state (threshold key, count above it, count equal to it)
//   oniris_vae_loss_topk_bwd     one pass: g * 2 d w / k with w from the saved state
// Operands are addressed by element strides in a loop order the caller chooses (up to 5 loop dimensions; 64-bit counts and
// offsets), or as flat 16-byte-aligned arrays (stride == NULL: 16 bytes per lane).  Float sums: a lane adds at most 64 terms in a
// row, chunks meet pairwise (a binary counter of partial sums), lanes and workgroups meet in fixed trees; no float atomic
// anywhere.  Counts are integers and do use LDS / global atomics: integer addition is exact in any order.  Two runs give the same
// bits.  Nothing here is contracted into an fma: the keys of the selection must be the separately rounded (r - t) * (r - t), and
// the fused kernels must give the same bits whichever sums are switched on.
#pragma clang fp contract(off)
#include "oniris.h"
#include "common.h"

#define VL_THREADS 256
#define VL_PER 4
#define VL_TILE (VL_THREADS * VL_PER)
#define VL_FLUSH 16               // tiles between two flushes of a lane's running sum: 16 x 4 = 64 terms
#define VL_LEVELS 20              // binary counter of chunk sums: 2^20 chunks of 64 terms per lane
#define VL_MAXT 6
#define VL_MAX_GRID (1 << 20)     // workgroups x VL_TILE stays below 2^31 (the first tile of a workgroup is split in 32 bits)
#define VL_MAX_DIM 0x7fffefffLL   // a loop dimension + VL_TILE stays below 2^31 (the magic-number division below)

struct VlIter {
  long long n, ntiles;
  int nd;                             // loop dimensions, outermost first, in [5 - nd, 5)
  int strided;
  unsigned size[5], mul[5], sh[5];    // x / size = (mulhi(x, mul) + x) >> sh for x < 2^31
  unsigned step[5];                   // gridDim.x * VL_TILE elements as loop coordinates (the outermost one unbounded)
  long long stride[VL_MAXT][5];
};

static int vl_build(VlIter& it, int nd, const long long* size, const long long* stride, int nt, int grid_cap, int* grid, const char* what) {
  ONIRIS_CHECK_ARG(nd >= 1 && nd <= 5 && size && nt <= VL_MAXT && grid_cap >= 1, "%s: bad layout arguments", what);
  memset(&it, 0, sizeof(it));
  long long n = 1;
  for (int k = 0; k < nd; ++k) {
    ONIRIS_CHECK_ARG(size[k] >= 1, "%s: empty dimension", what);
    ONIRIS_CHECK_ARG(n <= (1LL << 62) / size[k], "%s: too many elements", what);
    n *= size[k];
  }
  it.n = n;
  it.ntiles = (n + VL_TILE - 1) / VL_TILE;
  it.nd = nd;
  it.strided = stride != nullptr;
  const long long g = it.ntiles < grid_cap ? it.ntiles : grid_cap;
  *grid = (int)(g < VL_MAX_GRID ? g : VL_MAX_GRID);
  ONIRIS_CHECK_ARG(it.ntiles / *grid < ((long long)VL_FLUSH << VL_LEVELS), "%s: %lld elements over %d workgroups", what, n, *grid);
  for (int k = 0; k < 5; ++k) { it.size[k] = 1; it.mul[k] = 1; it.sh[k] = 0; }
  if (!stride) return ONIRIS_OK;
  unsigned long long rest = (unsigned long long)*grid * VL_TILE;
  for (int k = nd - 1; k >= 0; --k) {
    const int s = 5 - nd + k;
    ONIRIS_CHECK_ARG(size[k] <= VL_MAX_DIM, "%s: a strided dimension of %lld elements (at most %lld)", what, size[k], VL_MAX_DIM);
    const unsigned long long d = (unsigned long long)size[k];
    it.size[s] = (unsigned)d;
    int sh = 0;
    while ((1ULL << sh) < d) ++sh;
    it.sh[s] = (unsigned)sh;
    it.mul[s] = (unsigned)((((1ULL << sh) - d) << 32) / d + 1);
    if (k > 0) { it.step[s] = (unsigned)(rest % d); rest /= d; }
    else it.step[s] = (unsigned)rest;                       // < 2^31: never wraps
    for (int t = 0; t < nt; ++t) it.stride[t][s] = stride[(size_t)t * nd + k];
  }
  return ONIRIS_OK;
}

#ifdef __HIPCC__
__device__ __forceinline__ unsigned vl_div(unsigned x, unsigned mul, unsigned sh) { return (__umulhi(x, mul) + x) >> sh; }

// loop coordinates of one workgroup's current tile; advanced by the grid stride without a division
struct VlPos {
  unsigned c[5];
  __device__ __forceinline__ void init(const VlIter& it) {
    unsigned x = blockIdx.x * (unsigned)VL_TILE;
#pragma unroll
    for (int k = 4; k > 0; --k) {
      const unsigned q = vl_div(x, it.mul[k], it.sh[k]);
      c[k] = x - q * it.size[k];
      x = q;
    }
    c[0] = x;
  }
  __device__ __forceinline__ void advance(const VlIter& it) {
    unsigned carry = 0;
#pragma unroll
    for (int k = 4; k > 0; --k) {
      unsigned v = c[k] + it.step[k] + carry;
      carry = v >= it.size[k];
      c[k] = carry ? v - it.size[k] : v;
    }
    c[0] += it.step[0] + carry;
  }
  // element offsets of element r (< VL_TILE) of the tile in NT tensors
  template <int NT>
  __device__ __forceinline__ void offsets(const VlIter& it, unsigned r, long long (&off)[NT]) const {
#pragma unroll
    for (int t = 0; t < NT; ++t) off[t] = 0;
    unsigned q = r;
#pragma unroll
    for (int k = 4; k >= 0; --k) {
      if (k < 5 - it.nd) continue;
      unsigned x = c[k] + q;
      if (k > 0) {
        q = vl_div(x, it.mul[k], it.sh[k]);
        x -= q * it.size[k];
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) off[t] += (long long)x * it.stride[t][k];
    }
  }
};

// Pairwise meeting of chunk sums: push() is a binary increment, level l holds the sum of 2^l chunks or nothing.
template <int NS>
struct VlAcc {
  float run[NS], lvl[NS][VL_LEVELS];
  unsigned cnt, fill;
  __device__ __forceinline__ void init() {
    cnt = fill = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      run[s] = 0.f;
#pragma unroll
      for (int l = 0; l < VL_LEVELS; ++l) lvl[s][l] = 0.f;
    }
  }
  __device__ __forceinline__ void flush() {
    bool carry = true;
#pragma unroll
    for (int l = 0; l < VL_LEVELS; ++l) {
      const bool occ = (cnt >> l) & 1u;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (carry && occ) { run[s] = lvl[s][l] + run[s]; lvl[s][l] = 0.f; }
        else if (carry) lvl[s][l] = run[s];
      }
      carry = carry && occ;
    }
    ++cnt;
    fill = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) run[s] = 0.f;
  }
  // v[s] = the pairwise sum of one tile's (at most 4) terms
  __device__ __forceinline__ void add(const float (&v)[NS]) {
#pragma unroll
    for (int s = 0; s < NS; ++s) run[s] = run[s] + v[s];
    if (++fill == VL_FLUSH) flush();
  }
  // the workgroup's sum in thread 0 (red: 4 x NS floats of LDS)
  __device__ __forceinline__ void total(float (&out)[NS], float* red) {
    flush();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      float v = 0.f;
#pragma unroll
      for (int l = 0; l < VL_LEVELS; ++l) v = v + lvl[s][l];
      v = wave_sum(v);
      if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * NS + s] = v;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NS; ++s) out[s] = (red[s] + red[NS + s]) + (red[2 * NS + s] + red[3 * NS + s]);
  }
};

__device__ __forceinline__ float vl_get(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// ---- fused pointwise losses ----------------------------------------------------------------------------------------------------
struct VlFwdArgs {
  VlIter it;
  const float *mean, *logvar, *target;
  float* part;
  int which;
  float inv_n;
};

__device__ __forceinline__ void vl_fwd_elem(int which, float mu, float lv, float tg, float (&term)[3]) {
  const float d = mu - tg;
  const float dd = d * d;
  term[0] = (which & 1) ? (lv + dd * expf(-lv)) * 0.5f + 0.918f : 0.f;
  term[1] = fabsf(d);
  term[2] = dd;
}

template <bool STRIDED>
__global__ __launch_bounds__(VL_THREADS) void vl_fwd_kernel(VlFwdArgs a) {
  __shared__ float red[12];
  const int t = threadIdx.x;
  const bool gauss = a.which & 1;
  VlAcc<3> acc;
  acc.init();
  VlPos pos;
  if constexpr (STRIDED) pos.init(a.it);
  for (long long tile = blockIdx.x; tile < a.it.ntiles; tile += gridDim.x) {
    float term[VL_PER][3];
#pragma unroll
    for (int j = 0; j < VL_PER; ++j) term[j][0] = term[j][1] = term[j][2] = 0.f;
    if constexpr (STRIDED) {
#pragma unroll
      for (int j = 0; j < VL_PER; ++j) {
        const unsigned r = j * VL_THREADS + t;
        if (tile * VL_TILE + r < a.it.n) {
          long long off[3];
          pos.offsets<3>(a.it, r, off);
          vl_fwd_elem(a.which, a.mean[off[0]], gauss ? a.logvar[off[1]] : 0.f, a.target[off[2]], term[j]);
        }
      }
      pos.advance(a.it);
    } else {
      const long long i = tile * VL_TILE + (long long)t * VL_PER;
      if (i + VL_PER <= a.it.n) {
        const float4 mu = *(const float4*)(a.mean + i), tg = *(const float4*)(a.target + i);
        float4 lv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gauss) lv = *(const float4*)(a.logvar + i);
#pragma unroll
        for (int j = 0; j < VL_PER; ++j) vl_fwd_elem(a.which, vl_get(mu, j), vl_get(lv, j), vl_get(tg, j), term[j]);
      } else {
#pragma unroll
        for (int j = 0; j < VL_PER; ++j)
          if (i + j < a.it.n) vl_fwd_elem(a.which, a.mean[i + j], gauss ? a.logvar[i + j] : 0.f, a.target[i + j], term[j]);
      }
    }
    float v[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) v[s] = (term[0][s] + term[1][s]) + (term[2][s] + term[3][s]);
    acc.add(v);
  }
  float tot[3];
  acc.total(tot, red);
  if (t == 0) {
#pragma unroll
    for (int s = 0; s < 3; ++s) a.part[(size_t)blockIdx.x * 3 + s] = ((a.which >> s) & 1) ? tot[s] * a.inv_n : 0.f;
  }
}

struct VlBwdArgs {
  VlIter it;
  const float *mean, *logvar, *target, *cot[3];
  float *dmean, *dlogvar, *dtarget;
  int which;
  float inv_n;
};

// coefficients: cg = cot_gauss / n, ch = cg / 2, cl = cot_l1 / n, cm = 2 cot_mse / n
__device__ __forceinline__ void vl_bwd_elem(int which, float cg, float ch, float cl, float cm, float mu, float lv, float tg, float& gm,
                                            float& glv) {
  const float d = mu - tg;
  gm = 0.f;
  glv = 0.f;
  if (which & 1) {
    const float de = d * expf(-lv);
    gm = cg * de;
    glv = ch * (1.f - d * de);
  }
  if (which & 2) gm = gm + cl * (d > 0.f ? 1.f : d < 0.f ? -1.f : d);     // sign(0) = 0, sign(NaN) = NaN
  if (which & 4) gm = gm + cm * d;
}

template <bool STRIDED>
__global__ __launch_bounds__(VL_THREADS) void vl_bwd_kernel(VlBwdArgs a) {
  const int t = threadIdx.x;
  int which = a.which;
#pragma unroll
  for (int s = 0; s < 3; ++s)
    if (!a.cot[s]) which &= ~(1 << s);
  const bool gauss = which & 1;
  const float cg = (which & 1) ? a.cot[0][0] * a.inv_n : 0.f, ch = cg * 0.5f;
  const float cl = (which & 2) ? a.cot[1][0] * a.inv_n : 0.f;
  const float cm = (which & 4) ? (a.cot[2][0] * 2.f) * a.inv_n : 0.f;
  VlPos pos;
  if constexpr (STRIDED) pos.init(a.it);
  for (long long tile = blockIdx.x; tile < a.it.ntiles; tile += gridDim.x) {
    if constexpr (STRIDED) {
#pragma unroll
      for (int j = 0; j < VL_PER; ++j) {
        const unsigned r = j * VL_THREADS + t;
        if (tile * VL_TILE + r < a.it.n) {
          long long off[6];
          pos.offsets<6>(a.it, r, off);
          float gm, glv;
          vl_bwd_elem(which, cg, ch, cl, cm, a.mean[off[0]], gauss ? a.logvar[off[1]] : 0.f, a.target[off[2]], gm, glv);
          if (a.dmean) a.dmean[off[3]] = gm;
          if (a.dlogvar) a.dlogvar[off[4]] = glv;
          if (a.dtarget) a.dtarget[off[5]] = -gm;
        }
      }
      pos.advance(a.it);
    } else {
      const long long i = tile * VL_TILE + (long long)t * VL_PER;
      if (i + VL_PER <= a.it.n) {
        const float4 mu = *(const float4*)(a.mean + i), tg = *(const float4*)(a.target + i);
        float4 lv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gauss) lv = *(const float4*)(a.logvar + i);
        float gm[4], glv[4];
#pragma unroll
        for (int j = 0; j < VL_PER; ++j) vl_bwd_elem(which, cg, ch, cl, cm, vl_get(mu, j), vl_get(lv, j), vl_get(tg, j), gm[j], glv[j]);
        if (a.dmean) *(float4*)(a.dmean + i) = make_float4(gm[0], gm[1], gm[2], gm[3]);
        if (a.dlogvar) *(float4*)(a.dlogvar + i) = make_float4(glv[0], glv[1], glv[2], glv[3]);
        if (a.dtarget) *(float4*)(a.dtarget + i) = make_float4(-gm[0], -gm[1], -gm[2], -gm[3]);
      } else {
#pragma unroll
        for (int j = 0; j < VL_PER; ++j)
          if (i + j < a.it.n) {
            float gm, glv;
            vl_bwd_elem(which, cg, ch, cl, cm, a.mean[i + j], gauss ? a.logvar[i + j] : 0.f, a.target[i + j], gm, glv);
            if (a.dmean) a.dmean[i + j] = gm;
            if (a.dlogvar) a.dlogvar[i + j] = glv;
            if (a.dtarget) a.dtarget[i + j] = -gm;
          }
      }
    }
  }
}

// ---- worst-k%: radix select over the keys (bit pattern of e, sign cleared), digits of 11 | 10 | 10 bits ------------------------
#define VL_BINS0 2048
#define VL_BINS 1024
__device__ __forceinline__ unsigned vl_key(float e) { return __float_as_uint(e) & 0x7fffffffu; }

// One count per active lane into an LDS histogram.  Squared errors share a handful of exponents, and equal inputs (a saturated or
// quantised frame, recon == target) share one key: the lanes that agree with the wave's first active lane are counted by that lane
// in ONE atomic of their number, the others add 1 each.  Call from wave-uniform control flow.
__device__ __forceinline__ void vl_hist_add(unsigned* h, unsigned bin, bool active) {
  const unsigned long long act = __ballot(active);
  if (!act) return;
  const int lead = __ffsll((long long)act) - 1;
  const unsigned b0 = (unsigned)__shfl((int)bin, lead);
  const bool same = active && bin == b0;
  const unsigned long long sm = __ballot(same);
  if (same) {
    if ((int)(threadIdx.x & 63) == lead) atomicAdd(&h[b0], (unsigned)__popcll(sm));
  } else if (active) {
    atomicAdd(&h[bin], 1u);
  }
}

template <int NB>
__device__ __forceinline__ void vl_hist_flush(const unsigned* h, unsigned* g) {
  __syncthreads();
  for (int b = threadIdx.x; b < NB; b += VL_THREADS) {
    const unsigned v = h[b];
    if (v) atomicAdd(&g[b], v);
  }
}

struct VlKeysArgs {
  VlIter it;
  const float *recon, *target;
  float* e;
  unsigned* hist;
};

template <bool STRIDED>
__global__ __launch_bounds__(VL_THREADS) void vl_topk_keys_kernel(VlKeysArgs a) {
  __shared__ unsigned h[VL_BINS0];
  const int t = threadIdx.x;
  for (int b = t; b < VL_BINS0; b += VL_THREADS) h[b] = 0;
  __syncthreads();
  VlPos pos;
  if constexpr (STRIDED) pos.init(a.it);
  for (long long tile = blockIdx.x; tile < a.it.ntiles; tile += gridDim.x) {
    float e[VL_PER];
    bool ok[VL_PER];
    if constexpr (STRIDED) {
#pragma unroll
      for (int j = 0; j < VL_PER; ++j) {
        const unsigned r = j * VL_THREADS + t;
        const long long i = tile * VL_TILE + r;
        ok[j] = i < a.it.n;
        e[j] = 0.f;
        if (ok[j]) {
          long long off[2];
          pos.offsets<2>(a.it, r, off);
          const float d = a.recon[off[0]] - a.target[off[1]];
          e[j] = d * d;
          a.e[i] = e[j];
        }
      }
      pos.advance(a.it);
    } else {
      const long long i = tile * VL_TILE + (long long)t * VL_PER;
      if (i + VL_PER <= a.it.n) {
        const float4 r = *(const float4*)(a.recon + i), g = *(const float4*)(a.target + i);
#pragma unroll
        for (int j = 0; j < VL_PER; ++j) {
          const float d = vl_get(r, j) - vl_get(g, j);
          e[j] = d * d;
          ok[j] = true;
        }
        *(float4*)(a.e + i) = make_float4(e[0], e[1], e[2], e[3]);
      } else {
#pragma unroll
        for (int j = 0; j < VL_PER; ++j) {
          ok[j] = i + j < a.it.n;
          e[j] = 0.f;
          if (ok[j]) {
            const float d = a.recon[i + j] - a.target[i + j];
            e[j] = d * d;
            a.e[i + j] = e[j];
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < VL_PER; ++j) vl_hist_add(h, vl_key(e[j]) >> 20, ok[j]);
  }
  vl_hist_flush<VL_BINS0>(h, a.hist);
}

// state: [0] the key prefix fixed so far, [1] elements above it, [2] elements that match it
template <bool LAST>
__global__ __launch_bounds__(VL_THREADS) void vl_topk_count_kernel(const float* __restrict__ e, long long n, long long ntiles,
                                                                   const unsigned* __restrict__ state, unsigned* hist,
                                                                   float* __restrict__ part) {
  __shared__ unsigned h[VL_BINS];
  __shared__ float red[4];
  const int t = threadIdx.x;
  for (int b = t; b < VL_BINS; b += VL_THREADS) h[b] = 0;
  __syncthreads();
  constexpr int SHIFT = LAST ? 10 : 20;
  const unsigned prefix = state[0] >> SHIFT;
  VlAcc<1> acc;
  acc.init();
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long i = tile * VL_TILE + (long long)t * VL_PER;
    float v[VL_PER];
    bool ok[VL_PER];
    if (i + VL_PER <= n) {
      const float4 x = *(const float4*)(e + i);
#pragma unroll
      for (int j = 0; j < VL_PER; ++j) { v[j] = vl_get(x, j); ok[j] = true; }
    } else {
#pragma unroll
      for (int j = 0; j < VL_PER; ++j) { ok[j] = i + j < n; v[j] = ok[j] ? e[i + j] : 0.f; }
    }
    float above[VL_PER];
#pragma unroll
    for (int j = 0; j < VL_PER; ++j) {
      const unsigned key = vl_key(v[j]);
      vl_hist_add(h, (key >> (SHIFT - 10)) & (VL_BINS - 1), ok[j] && (key >> SHIFT) == prefix);
      above[j] = (ok[j] && (key >> SHIFT) > prefix) ? v[j] : 0.f;
    }
    if constexpr (LAST) {
      const float s[1] = {(above[0] + above[1]) + (above[2] + above[3])};
      acc.add(s);
    }
  }
  if constexpr (LAST) {
    float tot[1];
    acc.total(tot, red);
    if (t == 0) part[blockIdx.x] = tot[0];
  }
  vl_hist_flush<VL_BINS>(h, hist);
}

// One workgroup.  `need` = k - (elements above the prefix) is the rank of the threshold among the elements of this histogram,
// counted from the top bin: the digit is the bin d with count(bins > d) < need <= count(bins >= d).  LAST: the loss is
// (sum of e above the threshold + (k - count_gt) e_k) / k, where the sum is the partials of the last count pass (everything above
// the 21-bit prefix) plus count x value of the bins above d (a bin of the last digit is one key, so one value), in double.
template <int NB, bool LAST>
__global__ __launch_bounds__(VL_THREADS) void vl_topk_select_kernel(const unsigned* __restrict__ hist, int shift, unsigned long long k,
                                                                    unsigned* state, const float* __restrict__ part, int P,
                                                                    float* __restrict__ loss) {
  constexpr int PER = NB / VL_THREADS;
  __shared__ unsigned long long cs[VL_THREADS];
  __shared__ unsigned sel[3];
  __shared__ double ds[VL_THREADS];
  const int t = threadIdx.x;
  const unsigned prefix = state[0], gt = state[1];
  unsigned hv[PER];
  unsigned long long sum = 0;
#pragma unroll
  for (int d = 0; d < PER; ++d) { hv[d] = hist[t * PER + d]; sum += hv[d]; }
  cs[t] = sum;
  __syncthreads();
  unsigned long long above = 0;
  for (int u = t + 1; u < VL_THREADS; ++u) above += cs[u];
  const unsigned long long need = k - gt;
  if (above < need && need <= above + sum) {
    int d = PER - 1;
    for (; d > 0; --d) {
      if (need <= above + hv[d]) break;
      above += hv[d];
    }
    sel[0] = (unsigned)(t * PER + d);
    sel[1] = gt + (unsigned)above;
    sel[2] = hv[d];
  }
  __syncthreads();
  const unsigned digit = sel[0], key = prefix | (digit << shift);
  if constexpr (LAST) {
    double s = 0.0;
    for (int p = t; p < P; p += VL_THREADS) s += (double)part[p];
#pragma unroll
    for (int d = 0; d < PER; ++d) {
      const unsigned b = t * PER + d;
      if (b > digit && hv[d]) s += (double)hv[d] * (double)__uint_as_float(prefix | b);
    }
    ds[t] = s;
    __syncthreads();
    for (int w = VL_THREADS / 2; w > 0; w >>= 1) {
      if (t < w) ds[t] = ds[t] + ds[t + w];
      __syncthreads();
    }
    if (t == 0) loss[0] = (float)((ds[0] + (double)(k - sel[1]) * (double)__uint_as_float(key)) / (double)k);
  }
  if (t == 0) { state[0] = key; state[1] = sel[1]; state[2] = sel[2]; }
}

struct VlTopkBwdArgs {
  VlIter it;
  const float *recon, *target, *g;
  const unsigned* state;
  float *drecon, *dtarget;
  float two_over_k;
  unsigned k;
};

__device__ __forceinline__ float vl_topk_grad(float r, float g, unsigned thr, float c, float ct) {
  const float d = r - g;
  const unsigned key = vl_key(d * d);
  return key > thr ? c * d : key == thr ? ct * d : 0.f;
}

template <bool STRIDED>
__global__ __launch_bounds__(VL_THREADS) void vl_topk_bwd_kernel(VlTopkBwdArgs a) {
  const int t = threadIdx.x;
  const unsigned thr = a.state[0];
  const float c = a.g[0] * a.two_over_k;
  const float ct = c * ((float)(a.k - a.state[1]) / (float)a.state[2]);       // the tie weight (k - count_gt) / count_eq
  VlPos pos;
  if constexpr (STRIDED) pos.init(a.it);
  for (long long tile = blockIdx.x; tile < a.it.ntiles; tile += gridDim.x) {
    if constexpr (STRIDED) {
#pragma unroll
      for (int j = 0; j < VL_PER; ++j) {
        const unsigned r = j * VL_THREADS + t;
        if (tile * VL_TILE + r < a.it.n) {
          long long off[4];
          pos.offsets<4>(a.it, r, off);
          const float v = vl_topk_grad(a.recon[off[0]], a.target[off[1]], thr, c, ct);
          if (a.drecon) a.drecon[off[2]] = v;
          if (a.dtarget) a.dtarget[off[3]] = -v;
        }
      }
      pos.advance(a.it);
    } else {
      const long long i = tile * VL_TILE + (long long)t * VL_PER;
      if (i + VL_PER <= a.it.n) {
        const float4 r = *(const float4*)(a.recon + i), g = *(const float4*)(a.target + i);
        float v[VL_PER];
#pragma unroll
        for (int j = 0; j < VL_PER; ++j) v[j] = vl_topk_grad(vl_get(r, j), vl_get(g, j), thr, c, ct);
        if (a.drecon) *(float4*)(a.drecon + i) = make_float4(v[0], v[1], v[2], v[3]);
        if (a.dtarget) *(float4*)(a.dtarget + i) = make_float4(-v[0], -v[1], -v[2], -v[3]);
      } else {
#pragma unroll
        for (int j = 0; j < VL_PER; ++j)
          if (i + j < a.it.n) {
            const float v = vl_topk_grad(a.recon[i + j], a.target[i + j], thr, c, ct);
            if (a.drecon) a.drecon[i + j] = v;
            if (a.dtarget) a.dtarget[i + j] = -v;
          }
      }
    }
  }
}
#endif

// ---- entry points --------------------------------------------------------------------------------------------------------------
static bool vl_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int oniris_vae_loss_fwd(const float* mean, const float* logvar, const float* target, int which, int nd,
                                   const long long* size, const long long* stride, float* part, int max_blocks, int* blocks,
                                   oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(mean && target && part && blocks && which >= 1 && which <= 7, "vae_loss_fwd: bad arguments");
  ONIRIS_CHECK_ARG(!(which & 1) || logvar, "vae_loss_fwd: the Gaussian loss needs logvar");
  ONIRIS_CHECK_ARG(stride || (vl_aligned(mean) && vl_aligned(target) && vl_aligned(logvar)), "vae_loss_fwd: flat operands must be 16-byte aligned");
  VlFwdArgs a;
  int grid;
  if (int rc = vl_build(a.it, nd, size, stride, 3, max_blocks, &grid, "vae_loss_fwd")) return rc;
  a.mean = mean; a.logvar = logvar; a.target = target; a.part = part; a.which = which; a.inv_n = (float)(1.0 / (double)a.it.n);
  *blocks = grid;
  if (stride) ONIRIS_KLAUNCH(vl_fwd_kernel<true>, dim3(grid), dim3(VL_THREADS), 0, (hipStream_t)stream, a);
  else ONIRIS_KLAUNCH(vl_fwd_kernel<false>, dim3(grid), dim3(VL_THREADS), 0, (hipStream_t)stream, a);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_vae_loss_bwd(const float* mean, const float* logvar, const float* target, int which, int nd,
                                   const long long* size, const long long* stride, const float* cot_gauss, const float* cot_l1,
                                   const float* cot_mse, float* dmean, float* dlogvar, float* dtarget, int max_blocks,
                                   oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(mean && target && which >= 1 && which <= 7 && (dmean || dlogvar || dtarget), "vae_loss_bwd: bad arguments");
  ONIRIS_CHECK_ARG(!(which & 1) || logvar, "vae_loss_bwd: the Gaussian loss needs logvar");
  ONIRIS_CHECK_ARG(stride || (vl_aligned(mean) && vl_aligned(target) && vl_aligned(logvar) && vl_aligned(dmean) && vl_aligned(dlogvar) &&
                              vl_aligned(dtarget)), "vae_loss_bwd: flat operands must be 16-byte aligned");
  VlBwdArgs a;
  int grid;
  if (int rc = vl_build(a.it, nd, size, stride, 6, max_blocks, &grid, "vae_loss_bwd")) return rc;
  a.mean = mean; a.logvar = logvar; a.target = target; a.cot[0] = cot_gauss; a.cot[1] = cot_l1; a.cot[2] = cot_mse;
  a.dmean = dmean; a.dlogvar = dlogvar; a.dtarget = dtarget; a.which = which; a.inv_n = (float)(1.0 / (double)a.it.n);
  if (stride) ONIRIS_KLAUNCH(vl_bwd_kernel<true>, dim3(grid), dim3(VL_THREADS), 0, (hipStream_t)stream, a);
  else ONIRIS_KLAUNCH(vl_bwd_kernel<false>, dim3(grid), dim3(VL_THREADS), 0, (hipStream_t)stream, a);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_vae_loss_topk_keys(const float* recon, const float* target, int nd, const long long* size,
                                         const long long* stride, float* e, unsigned* hist, int max_blocks, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(recon && target && e && hist && vl_aligned(e), "vae_loss_topk_keys: bad arguments");
  ONIRIS_CHECK_ARG(stride || (vl_aligned(recon) && vl_aligned(target)), "vae_loss_topk_keys: flat operands must be 16-byte aligned");
  VlKeysArgs a;
  int grid;
  if (int rc = vl_build(a.it, nd, size, stride, 2, max_blocks, &grid, "vae_loss_topk_keys")) return rc;
  ONIRIS_CHECK_ARG(a.it.n <= 0xffffffffLL, "vae_loss_topk_keys: %lld elements (the counts are 32-bit)", a.it.n);
  a.recon = recon; a.target = target; a.e = e; a.hist = hist;
  if (stride) ONIRIS_KLAUNCH(vl_topk_keys_kernel<true>, dim3(grid), dim3(VL_THREADS), 0, (hipStream_t)stream, a);
  else ONIRIS_KLAUNCH(vl_topk_keys_kernel<false>, dim3(grid), dim3(VL_THREADS), 0, (hipStream_t)stream, a);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_vae_loss_topk_count(const float* e, long long n, int last, const unsigned* state, unsigned* hist, float* part,
                                          int max_blocks, int* blocks, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(e && vl_aligned(e) && n >= 1 && n <= 0xffffffffLL && state && hist && max_blocks >= 1 && blocks && (!last || part),
                   "vae_loss_topk_count: bad arguments");
  const long long ntiles = (n + VL_TILE - 1) / VL_TILE;
  long long g = ntiles < max_blocks ? ntiles : max_blocks;
  if (g > VL_MAX_GRID) g = VL_MAX_GRID;
  *blocks = (int)g;
  if (last) ONIRIS_KLAUNCH(vl_topk_count_kernel<true>, dim3((unsigned)g), dim3(VL_THREADS), 0, (hipStream_t)stream, e, n, ntiles, state, hist, part);
  else ONIRIS_KLAUNCH(vl_topk_count_kernel<false>, dim3((unsigned)g), dim3(VL_THREADS), 0, (hipStream_t)stream, e, n, ntiles, state, hist, part);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_vae_loss_topk_select(const unsigned* hist, int digit, long long k, unsigned* state, const float* part, int P,
                                           float* loss, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(hist && state && digit >= 0 && digit <= 2 && k >= 1 && k <= 0xffffffffLL, "vae_loss_topk_select: bad arguments");
  ONIRIS_CHECK_ARG(digit < 2 || (part && P >= 1 && loss), "vae_loss_topk_select: the last digit needs the partial sums and the loss");
  const hipStream_t s = (hipStream_t)stream;
  const unsigned long long kk = (unsigned long long)k;
  const auto k0 = vl_topk_select_kernel<VL_BINS0, false>;
  const auto k1 = vl_topk_select_kernel<VL_BINS, false>;
  const auto k2 = vl_topk_select_kernel<VL_BINS, true>;
  if (digit == 0) ONIRIS_KLAUNCH(k0, dim3(1), dim3(VL_THREADS), 0, s, hist, 20, kk, state, part, P, loss);
  else if (digit == 1) ONIRIS_KLAUNCH(k1, dim3(1), dim3(VL_THREADS), 0, s, hist, 10, kk, state, part, P, loss);
  else ONIRIS_KLAUNCH(k2, dim3(1), dim3(VL_THREADS), 0, s, hist, 0, kk, state, part, P, loss);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}

extern "C" int oniris_vae_loss_topk_bwd(const float* recon, const float* target, int nd, const long long* size,
                                        const long long* stride, const unsigned* state, const float* g, long long k, float* drecon,
                                        float* dtarget, int max_blocks, oniris_stream_t stream) {
  ONIRIS_CHECK_ARG(recon && target && state && g && k >= 1 && k <= 0xffffffffLL && (drecon || dtarget), "vae_loss_topk_bwd: bad arguments");
  ONIRIS_CHECK_ARG(stride || (vl_aligned(recon) && vl_aligned(target) && vl_aligned(drecon) && vl_aligned(dtarget)),
                   "vae_loss_topk_bwd: flat operands must be 16-byte aligned");
  VlTopkBwdArgs a;
  int grid;
  if (int rc = vl_build(a.it, nd, size, stride, 4, max_blocks, &grid, "vae_loss_topk_bwd")) return rc;
  a.recon = recon; a.target = target; a.g = g; a.state = state; a.drecon = drecon; a.dtarget = dtarget;
  a.two_over_k = (float)(2.0 / (double)k); a.k = (unsigned)k;
  if (stride) ONIRIS_KLAUNCH(vl_topk_bwd_kernel<true>, dim3(grid), dim3(VL_THREADS), 0, (hipStream_t)stream, a);
  else ONIRIS_KLAUNCH(vl_topk_bwd_kernel<false>, dim3(grid), dim3(VL_THREADS), 0, (hipStream_t)stream, a);
  ONIRIS_LAUNCH_CHECK();
  return ONIRIS_OK;
}
