"""float64 expectations for the fp32 verification kernels (csrc/fp32.hip through autoregressive_diffusion_amd/fp32.py)  --  TEST
INFRASTRUCTURE, CPU only.  tests/test_fp32_oracle.py shows that these expectations and their bounds see the faults they are for,
tests/test_fp32_stages_gpu.py holds the kernels to them.

CONV.  Value and, per element, the sum of the absolute values of its own terms, in float64 from float32 inputs: forward and data
gradient from tests/disc_cpu_restatement.py (conv_terms, dgrad_terms), the weight gradient here (wgrad_terms, which also counts
the non-zero terms of every element).  Element bound: (K + 4) u sum|terms|, u = 2^-24 -- a float32 sum of K products in ANY order
(tests/test_discriminator_gpu.py derives it); for the weight gradient K is the element's own number of non-zero terms and the
number of position chunks is added: the chunks' partial sums meet in atomics, one more rounding each.

POSITION PROBES for the weight gradient.  dW[co][ci][tap] = sum over positions p of dy[p][co] x[shift(p, tap)][ci].  x is zero
except at a short list of positions (every channel random there), dy is dense: an element of dW then has at most as many terms
as there are probe positions, and a position that the kernel drops, doubles or shifts changes it by the size of one of its few
terms.  The list: the first and the last position, the four corners of every image, the two positions on each side of every
multiple of the kernel's chunk of 4096 positions, and every position of the last group of 16 of each chunk.

ATTENTION.  reference(): a dense masked softmax in float64 for q (BH, Lq, D) against k, v (BH, Lk, D) under an ARBITRARY boolean
`allowed` (Lq, Lk), gradients by autograd.  The allowed matrices are built from the package's mask DEFINITIONS, not from the closed
form the kernel evaluates: train_allowed() = attention_masking.TrainingMask on token indices AND the dense expansion of the block
table ops.train_mask_table returns; causal_allowed() = attention_masking.InferenceMask with the query index shifted by the cached
frames.
model_f32(): the same operations in float32 with the kernel's roundings -- scores as a sequential sum over the channels, keys in
chunks of 64 with the running maximum and the rescaling of the running sums, the exponential as exp2(x log2 e), P V accumulated key
by key (dq key by key, dk and dv query by query), lse = m + log2(l) ln 2 and P = exp(s scale - lse) in the backward pass.  It is
the yardstick of the random-input bounds: RANDOM_BOUND_FACTOR x its worst row against float64.

COUNT PROBES (as tests/attention_probes.py, for this layout).  q = k = one constant vector per head: every score is equal, the
softmax is uniform over the allowed set.  v of key j is one-hot in channel j % D', D' = min(D, 64); dO of query i is n_i (its
number of allowed keys) one-hot in channel (i + D'/2) % D'.  Row i of `out` is (allowed keys per class) / n_i, row j of dv the
number of queries that attend key j, per class: a wrong (query, key) pair moves `out` by 1 / n_i >= 1 / Lk and dv by 1.
"""
import math

import numpy as np
import torch

import disc_cpu_restatement as R
from attention_probes import RANDOM_BOUND_FACTOR      # noqa: F401  (4: the factor of every random-input row bound of the suite)

U = 2.0 ** -24               # unit roundoff of float32
WGRAD_CHUNK = 4096           # positions per blockIdx.z of wgrad_f32_kernel (oniris_wgrad_f32)
WGRAD_GROUP = 16             # positions per LDS pass of that kernel
KEY_CHUNK = 64               # rows of the streamed side per LDS pass of the attention kernels
COUNT_OUT_TOL = 2.0 ** -20   # count probes, out: every exp argument is exactly 0 and l an exact integer; a reciprocal and a product remain
COUNT_DV_TOL = 2.0 ** -6     # count probes, dv (absolute; a wrong pair moves it by 1) and dq / dk (relative to the largest |dv|)
MODEL_DV_TOL = 2.0 ** -8     # what model_f32 alone has to stay under on the count probes
FAULT_MARGIN = 3.0           # a planted fault must exceed its bound this many times (the rule of tests/test_attention_probes.py)

conv_terms = R.conv_terms
dgrad_terms = R.dgrad_terms


# ----------------------------------------------------------------------------------------------------------------------
# convolution

def wgrad_terms(x, dy, k):
    """d weight of conv2d(x, w, padding=k // 2) at dy, x (N, Cin, H, W), dy (N, Cout, H, W), in their dtype:
    -> (dW (Cout, Cin, k, k), its sum of absolute terms, per element the number of non-zero terms)."""
    N, Cin, H, W = x.shape
    pad = k // 2
    xp = torch.nn.functional.pad(x, (pad, pad, pad, pad))
    nzx, nzy = (xp != 0).to(x.dtype), (dy != 0).to(x.dtype)
    res = []
    for a, b in ((xp, dy), (xp.abs(), dy.abs()), (nzx, nzy)):
        res.append(torch.stack([torch.stack([torch.einsum("nchw,nohw->oc", a[:, :, ky:ky + H, kx:kx + W], b) for kx in range(k)], -1)
                                for ky in range(k)], -2))
    return res[0], res[1], res[2].round().long()


def element_bound(mag, K, extra=0):
    """(K + extra + 4) u sum|terms|; K a number or one per element."""
    K = torch.as_tensor(K, dtype=torch.float64)
    return (K + extra + 4) * U * mag.double()


def wgrad_chunks(npos):
    return (npos + WGRAD_CHUNK - 1) // WGRAD_CHUNK


def probe_positions(N, H, W):
    """The flat positions p = (n H + y) W + x of the position probes, sorted."""
    npos, HW = N * H * W, H * W
    pos = {0, npos - 1}
    for n in range(N):
        pos |= {n * HW, n * HW + W - 1, n * HW + (H - 1) * W, n * HW + HW - 1}
    for b in range(WGRAD_CHUNK, npos, WGRAD_CHUNK):
        pos |= {b - 2, b - 1, b, b + 1}
    for c in range(wgrad_chunks(npos)):
        lo, hi = c * WGRAD_CHUNK, min((c + 1) * WGRAD_CHUNK, npos)
        pos |= set(range(lo + (hi - lo - 1) // WGRAD_GROUP * WGRAD_GROUP, hi))
    return sorted(p for p in pos if 0 <= p < npos)


def position_probe(N, H, W, Cin, seed):
    """x (N, Cin, H, W) float32: zero except at probe_positions, random on every channel there."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.tensor(probe_positions(N, H, W))
    x = torch.zeros(N * H * W, Cin)
    x[pos] = torch.randn(len(pos), Cin, generator=g)
    return x.reshape(N, H, W, Cin).permute(0, 3, 1, 2).contiguous()


def position_weights(N, H, W, weights):
    """(N, 1, H, W) float tensor: 1 everywhere, weights[p] at flat position p -- multiplied into dy it drops (0) or doubles (2)
    the terms of position p in a weight gradient."""
    w = torch.ones(N * H * W)
    for p, v in weights.items():
        w[p] = v
    return w.reshape(N, 1, H, W)


# ----------------------------------------------------------------------------------------------------------------------
# masks, from the package's definitions

def train_allowed(T, P):
    """(2TP, 2TP) bool: TrainingMask(T, P) on token indices AND the block table of ops.train_mask_table(T, P) expanded block by
    block (blocks of 128 x 128 tokens; of P x P from 128-token frames on: the block size the table itself reports)."""
    from autoregressive_diffusion_amd import ops
    from edm2.attention.attention_masking import TrainingMask
    tab = ops.train_mask_table(T, P)
    assert tab is not None, f"no training mask table for T = {T}, P = {P}"
    num, idx, blk = tab
    L = 2 * T * P
    assert len(num) * blk == L
    listed = np.zeros((len(num), len(num)), dtype=bool)
    for i in range(len(num)):
        listed[i, idx[i, :num[i]]] = True
    tok = torch.arange(L)
    mod = TrainingMask(T, P)(None, None, tok[:, None], tok[None, :])
    return mod & torch.from_numpy(listed)[tok[:, None] // blk, tok[None, :] // blk]


def train_mask_mod_only(T, P):
    """TrainingMask alone (the fault 'mask_mod without the block table')."""
    from edm2.attention.attention_masking import TrainingMask
    tok = torch.arange(2 * T * P)
    return TrainingMask(T, P)(None, None, tok[:, None], tok[None, :])


def causal_allowed(q_frames, cached_frames, P):
    """(q_frames P, (cached + q_frames) P) bool: InferenceMask(P), the queries being the LAST q_frames frames of the keys."""
    from edm2.attention.attention_masking import InferenceMask
    qi = torch.arange(q_frames * P)[:, None] + cached_frames * P
    kj = torch.arange((cached_frames + q_frames) * P)[None, :]
    return InferenceMask(P)(None, None, qi, kj)


def dense_allowed(Lq, Lk):
    return torch.ones(Lq, Lk, dtype=torch.bool)


# ----------------------------------------------------------------------------------------------------------------------
# attention: float64 reference, float32 model

NAMES = ("out", "dq", "dk", "dv")


def reference(q, k, v, dO, allowed, scale=None):
    """float64 (out, dq, dk, dv) of softmax(scale q k^T over the allowed keys) v at the upstream gradient dO."""
    q, k, v = (z.detach().double().clone().requires_grad_(True) for z in (q, k, v))
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~allowed, float("-inf"))
    out = torch.softmax(s, dim=-1) @ v
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), dO.double())
    return dict(out=out.detach(), dq=dq, dk=dk, dv=dv)


def _fma(acc, a, b):
    """float32 acc + a b with ONE rounding: the product of two float32 is exact in float64."""
    return (acc.double() + a.double() * b.double()).float()


_LOG2E = torch.tensor(math.log2(math.e), dtype=torch.float32)
_LN2 = torch.tensor(math.log(2.0), dtype=torch.float32)
_NEG = -1e30


def _exp(x):
    return torch.exp2(x * _LOG2E)


def _dot_rows(a, b):
    """(BH, La, D), (BH, Lb, D) float32 -> (BH, La, Lb): sum over the channels one after the other, fused multiply-adds."""
    s = torch.zeros(a.shape[0], a.shape[1], b.shape[1], dtype=torch.float32)
    for c in range(a.shape[-1]):
        s = _fma(s, a[:, :, None, c], b[:, None, :, c])
    return s


def model_f32(q, k, v, dO, allowed, scale=None):
    """float32 (out, dq, dk, dv) with the roundings of attn_f32_fwd / _dq / _dkv (module docstring)."""
    q, k, v, dO = (z.detach().float() for z in (q, k, v, dO))
    BH, Lq, D = q.shape
    Lk = k.shape[1]
    scale = torch.tensor(1.0 / math.sqrt(D) if scale is None else scale, dtype=torch.float32)
    raw = _dot_rows(q, k)
    s = raw * scale
    m = torch.full((BH, Lq), _NEG, dtype=torch.float32)
    l = torch.zeros(BH, Lq, dtype=torch.float32)
    acc = torch.zeros(BH, Lq, D, dtype=torch.float32)
    for k0 in range(0, Lk, KEY_CHUNK):
        k1 = min(k0 + KEY_CHUNK, Lk)
        ok = allowed[:, k0:k1]
        sc = torch.where(ok, s[:, :, k0:k1], torch.tensor(_NEG))
        mn = torch.maximum(m, sc.amax(-1))
        p = torch.where(ok, _exp(sc - mn[..., None]), torch.tensor(0.0))
        corr = _exp(m - mn)
        l = l * corr + p.sum(-1)
        m = mn
        acc = acc * corr[..., None]
        for j in range(k1 - k0):
            acc = _fma(acc, p[:, :, j, None], v[:, None, k0 + j, :])
    has = l > 0
    out = acc * torch.where(has, 1.0 / l, torch.tensor(0.0))[..., None]
    lse = torch.where(has, m + torch.log2(l) * _LN2, torch.tensor(_NEG))
    delta = (dO * out).sum(-1)
    p = torch.where(allowed, _exp(_fma(-lse[..., None], raw, scale)), torch.tensor(0.0))
    ds = p * (_dot_rows(dO, v) - delta[..., None]) * scale
    dq = torch.zeros_like(q)
    for j in range(Lk):
        dq = _fma(dq, ds[:, :, j, None], k[:, None, j, :])
    dk, dv = torch.zeros_like(k), torch.zeros_like(v)
    for i in range(Lq):
        dv = _fma(dv, p[:, i, :, None], dO[:, None, i, :])
        dk = _fma(dk, ds[:, i, :, None], q[:, None, i, :])
    return dict(out=out, dq=dq, dk=dk, dv=dv)


def random_inputs(BH, Lq, Lk, D, seed):
    """q, k ~ randn / D^0.25, v, dO ~ randn (float32)."""
    g = torch.Generator().manual_seed(seed)
    q, dO = torch.randn(BH, Lq, D, generator=g), torch.randn(BH, Lq, D, generator=g)
    k, v = torch.randn(BH, Lk, D, generator=g), torch.randn(BH, Lk, D, generator=g)
    return q / D ** 0.25, k / D ** 0.25, v, dO


def count_probe(BH, D, allowed, seed=0):
    """q, k, v, dO (float32) of the count probe under `allowed` (Lq, Lk)."""
    Lq, Lk = allowed.shape
    Dp = min(D, 64)
    g = torch.Generator().manual_seed(seed)
    const = torch.randn(BH, 1, D, generator=g)
    q, k = const.expand(BH, Lq, D).contiguous(), const.expand(BH, Lk, D).contiguous()
    v, dO = torch.zeros(BH, Lk, D), torch.zeros(BH, Lq, D)
    j, i = torch.arange(Lk), torch.arange(Lq)
    v[:, j, j % Dp] = 1.0
    dO[:, i, (i + Dp // 2) % Dp] = allowed.sum(1).float()
    return q, k, v, dO


def count_expectation(D, allowed):
    """(out (Lq, D), dv (Lk, D)) of a count probe from the counts themselves, float64."""
    Lq, Lk = allowed.shape
    Dp = min(D, 64)
    al = allowed.double()
    cls_k = torch.zeros(Lk, D, dtype=torch.float64)
    cls_k[torch.arange(Lk), torch.arange(Lk) % Dp] = 1.0
    cls_q = torch.zeros(Lq, D, dtype=torch.float64)
    cls_q[torch.arange(Lq), (torch.arange(Lq) + Dp // 2) % Dp] = 1.0
    return (al @ cls_k) / al.sum(1, keepdim=True), al.t() @ cls_q


def row_error(got, ref):
    """max|got - ref| / max|ref| over the channels of every row: (BH, L) float64."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape
    return (got - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-300)


def random_bounds(ref, model):
    """Per tensor: RANDOM_BOUND_FACTOR x the worst row of the float32 model against float64."""
    return {n: RANDOM_BOUND_FACTOR * float(row_error(model[n], ref[n]).max()) for n in NAMES}


# ----------------------------------------------------------------------------------------------------------------------
# the cases both test files use

TRAIN_COUNT_CASES = [(1, 256), (4, 64), (16, 16), (64, 4), (128, 2), (256, 2)]      # (P, T): fpb = 128, 32, 8, 2, 1 and P >= 128
CAUSAL_CASES = [(2, 3, 20), (2, 1, 9), (3, 0, 50)]                                  # (query frames, cached frames, P)
DENSE_CASE = (13, 70)                                                               # (Lq, Lk)
COUNT_BH, COUNT_D = 2, 64


def count_cases():
    """(id, mask name, kernel arguments, zero-argument builder of `allowed`) of every count-probe case."""
    cases = [(f"train-P{P}-T{T}", "train", dict(P=P, T=T), lambda P=P, T=T: train_allowed(T, P)) for P, T in TRAIN_COUNT_CASES]
    cases += [(f"causal-{tq}on{n}-P{P}", "causal", dict(P=P, q_frame_off=n), lambda tq=tq, n=n, P=P: causal_allowed(tq, n, P))
              for tq, n, P in CAUSAL_CASES]
    return cases + [("dense-13x70", "dense", {}, lambda: dense_allowed(*DENSE_CASE))]
