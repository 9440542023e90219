"""Probe inputs and float64 row references for the attention kernels  --  TEST INFRASTRUCTURE, CPU only.

The existing attention tests assert one relative L2 norm per tensor: a mask error on a few (query, key) pairs moves it by about
1e-4.  The helpers here make such an error move ONE ROW by a multiple of the row's own size, and measure rows one at a time.

Everything is in the packed layout ops.attention_train / ops.attention_eval take: x (N, P, 3C), channel = s * C + head * 64 + c
(s = 0, 1, 2: q, k, v), N = sequences * frames, a training sequence being (T clean, T noisy) frames.

COUNT PROBES.  Raw q and raw k of every token are one constant vector per head and the rope buffers are the identity
(inv_freq = 0, scale = 1), so every score is 8 and the softmax is uniform over the allowed set.  Raw v of key j is one-hot in
channel cls(j): row i of `out` then holds, per class, the NUMBER of allowed keys divided by the row's key count.  Classes:
    "frame":  cls(j) = frame index of j (mod 64)       "mod64":  cls(j) = j mod 64
The upstream gradient of query i is one-hot too, with value n_i = its number of allowed keys (rounded to bf16), so that every
query gives every key it attends the same weight P_ij * n_i = 1, wherever it sits in the sequence: row j of dv holds, per
class, the number of QUERIES that attend key j -- the transposed mask.  (With a unit gradient the weight is 1 / n_i, and a late
query's contribution to an early key drowns in the early queries'.)
dqkv is the gradient with respect to the RAW qkv: the adjoint of the per-head normalisation removes the component of dv along v
itself.  The frame class therefore puts the gradient of query i in channel cls(i) + 32: with at most 32 frames the channels of
v and of dO are disjoint and nothing is removed.  The mod-64 class keeps channel cls(i); the pairs with i = j (mod 64) are
invisible in its dv (not in its `out`) and are what the frame-class head sees.
dq and dk of a count probe are zero up to rounding: the rows of dS sum to zero and K is constant (dq), and dk is parallel to k,
which the normalisation adjoint removes.

REFERENCE.  reference() restates the op in float64 from the oracle's own functions (O.normalize, O.rope_apply) and a dense
masked softmax written out, with an ARBITRARY boolean `allowed` matrix; the gradient by autograd.  model_bf16() is the same in
float32 with the roundings the kernels make (bf16 q / k / v, bf16 P and dS as matrix operands, bf16 results): the noise model
the random-input bounds are taken from.
"""
import numpy as np
import torch

from oracle import oniris_oracle as O

D = 64                       # head dimension of the kernels under test
COUNT_TOL = 2.0 ** -6        # count-probe row bound (bf16 P, operands, result: <= 2^-9 relative each)
RANDOM_BOUND_FACTOR = 4.0    # random-input rows: this many times the modelled bf16 noise


def bfr(x):
    return x.to(torch.bfloat16).to(x.dtype)


def identity_rope():
    """rope_bufs under which O.rope_apply (and the kernels' tables) leave q and k unchanged: angle 0, xPos scale 1."""
    return torch.zeros(D // 2), torch.ones(D // 2)


def real_rope():
    """The rope buffers of the existing attention tests."""
    return 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D)), (torch.arange(0, D, 2) + 0.4 * D) / (1.4 * D)


def head_classes(heads, n_frames):
    """One class per head, 'frame' and 'mod64' alternating; 'mod64' alone past 32 frames (the frame class needs 32 channels for v
    and 32 for dO).  A one-head case is parametrised over the two classes by its caller."""
    if n_frames > 32:
        return ["mod64"] * heads
    return [("frame", "mod64")[h % 2] for h in range(heads)]


def token_classes(cls, n_frames, P):
    tok = np.arange(n_frames * P)
    return (tok // P) % 64 if cls == "frame" else tok % 64


def grad_channels(cls, n_frames, P):
    c = token_classes(cls, n_frames, P)
    return (c + 32) % 64 if cls == "frame" else c


def count_probe(n_seq, n_frames, P, classes, allowed=None, seed=0, frame_offset=None):
    """x (n_seq * n_frames, P, 3C) and dO (n_seq * n_frames, P, C), float32 holding bf16 values.
    allowed (L, L) bool: the TRUE mask, only used for the size n_i of the gradient of query i (None: n_i = 1).
    frame_offset (n_seq,): added to the frame index of the 'frame' class per sequence (FrameAttention: every frame is a sequence of
    its own and its class is its global index)."""
    heads = len(classes)
    C, L = heads * D, n_frames * P
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(n_seq, L, 3, heads, D)
    dO = torch.zeros(n_seq, L, heads, D)
    n_i = torch.ones(L) if allowed is None else bfr(torch.from_numpy(np.asarray(allowed)).sum(1).float())
    rows = torch.arange(L)
    for h, cls in enumerate(classes):
        const = bfr(torch.randn(D, generator=g))
        x[:, :, 0, h] = const
        x[:, :, 1, h] = const
        for b in range(n_seq):
            off = int(frame_offset[b]) if (frame_offset is not None and cls == "frame") else 0
            cv = torch.from_numpy((token_classes(cls, n_frames, P) + off) % 64)
            cg = torch.from_numpy((grad_channels(cls, n_frames, P) + off) % 64)
            x[b, rows, 2, h, cv] = 1.0
            dO[b, rows, h, cg] = n_i
    x = x.reshape(n_seq, n_frames, P, 3 * C).reshape(n_seq * n_frames, P, 3 * C)
    dO = dO.reshape(n_seq * n_frames, P, C)
    return x, dO


def random_inputs(N, P, heads, seed):
    """The randn / bf16-rounded inputs of the existing tests, packed layout."""
    g = torch.Generator().manual_seed(seed)
    return bfr(torch.randn(N, P, 3 * heads * D, generator=g)), bfr(torch.randn(N, P, heads * D, generator=g))


# ----------------------------------------------------------------------------------------------------------------------
# float64 reference

def _heads_view(t, n_seq, heads):
    """(N, P, heads*64) -> (n_seq, heads, frames, P, 64)."""
    N, P, _ = t.shape
    return t.reshape(n_seq, N // n_seq, P, heads, D).permute(0, 3, 1, 2, 4)


def _packed(t, N, P):
    """(n_seq, heads, L, 64) -> (N, P, heads*64)."""
    n_seq, heads, L, _ = t.shape
    return t.reshape(n_seq, heads, N // n_seq, P, D).permute(0, 2, 3, 1, 4).reshape(N, P, heads * D)


def prepared_qkv(x, n_seq, heads, rope, training, cache=None):
    """Normalised (and rotated) q, k, v (n_seq, heads, L, 64) of packed x, in x's dtype, on the autograd graph of x.
    cache: (k, v) (n_seq, heads, frames, P, 64), normalised and un-rotated, put in front of the new frames' (evaluation)."""
    C = x.shape[2] // 3
    q, k, v = (O.normalize(_heads_view(x[:, :, s * C:(s + 1) * C], n_seq, heads), dim=-1) for s in range(3))
    if cache is not None:
        k, v = torch.cat([cache[0].to(x.dtype), k], 2), torch.cat([cache[1].to(x.dtype), v], 2)
    if rope is not None:
        q, k = O.rope_apply(q, k, rope[0].float(), rope[1].float(), training)
        q, k = q.to(x.dtype), k.to(x.dtype)
    return tuple(z.reshape(n_seq, heads, -1, D) for z in (q, k, v))


def masked_softmax(q, k, allowed):
    """softmax(q k^T / sqrt(64)) over the allowed keys of every row, dense; allowed (Lq, Lk) bool tensor or None."""
    s = q @ k.transpose(-1, -2) / 8.0
    if allowed is not None:
        s = s.masked_fill(~allowed, float("-inf"))
    return torch.softmax(s, dim=-1)


def reference(x, dO, n_seq, heads, allowed, rope=None, training=True, cache=None):
    """float64: out (N, P, C) and, with dO, dqkv (N, P, 3C) of the attention core on packed x under `allowed`."""
    x = x.detach().double().clone().requires_grad_(dO is not None)
    N, P, _ = x.shape
    q, k, v = prepared_qkv(x, n_seq, heads, rope, training, cache)
    al = None if allowed is None else torch.as_tensor(np.asarray(allowed))
    out = _packed(masked_softmax(q, k, al) @ v, N, P)
    if dO is None:
        return out.detach(), None
    (dqkv,) = torch.autograd.grad(out, x, dO.double())
    return out.detach(), dqkv


def model_bf16(x, dO, n_seq, heads, allowed, rope=None, training=True):
    """float32 restatement with the kernels' roundings: q, k, v rounded to bf16 after normalisation and rotation; P and dS rounded
    to bf16 where they are matrix operands; out, dq, dk, dv and dqkv rounded to bf16; every sum in float32."""
    x = x.detach().float().clone().requires_grad_(True)
    N, P, _ = x.shape
    q0, k0, v0 = prepared_qkv(x, n_seq, heads, rope, training)
    q, k, v = (bfr(z.detach()) for z in (q0, k0, v0))
    al = None if allowed is None else torch.as_tensor(np.asarray(allowed))
    p = masked_softmax(q, k, al)
    out = bfr(bfr(p) @ v)
    go = _heads_view(dO.float(), n_seq, heads).reshape(out.shape)
    delta = (go * out).sum(-1, keepdim=True)
    ds = bfr(p * (go @ v.transpose(-1, -2) - delta))
    dq, dk, dv = bfr(ds @ k / 8.0), bfr(ds.transpose(-1, -2) @ q / 8.0), bfr(bfr(p).transpose(-1, -2) @ go)
    (dqkv,) = torch.autograd.grad([q0, k0, v0], x, [dq, dk, dv])
    return _packed(out, N, P), bfr(dqkv)


# ----------------------------------------------------------------------------------------------------------------------
# row metric

def split_dqkv(dqkv):
    C = dqkv.shape[-1] // 3
    return {"dq": dqkv[..., :C], "dk": dqkv[..., C:2 * C], "dv": dqkv[..., 2 * C:]}


def row_metric(got, ref, heads):
    """max|got - ref| / max|ref| over the 64 channels of one head, for every token row: (N, P, heads) float64."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    N, P, _ = ref.shape
    g, r = got.reshape(N, P, heads, D), ref.reshape(N, P, heads, D)
    return (g - r).abs().amax(-1) / r.abs().amax(-1).clamp_min(1e-300)


def worst_rows(got, ref, heads, frames_per_seq=1):
    """Per head: (worst row metric, its description).  got / ref (N, P, heads*64)."""
    m = row_metric(got, ref, heads)
    N, P, _ = m.shape
    res = []
    for h in range(heads):
        flat = int(m[:, :, h].argmax())
        n, pos = divmod(flat, P)
        res.append((float(m[n, pos, h]), f"head {h}, sequence {n // frames_per_seq}, frame {n % frames_per_seq}, position {pos}"))
    return res


def check_rows(name, got, ref, heads, bound, frames_per_seq=1, report=None):
    """Asserts every row of every head within `bound` (a number or one per head); the message names the worst row."""
    worst = worst_rows(got, ref, heads, frames_per_seq)
    bounds = bound if isinstance(bound, (list, tuple)) else [bound] * heads
    if report is not None:
        report[name] = max(w for w, _ in worst)
    bad = [f"{name}: row metric {w:.3e} > {b:.3e} at {where}" for (w, where), b in zip(worst, bounds) if not w <= b]
    assert not bad, "; ".join(bad)


def check_zero(name, got, scale, bound=COUNT_TOL):
    """dq / dk of a count probe: |got| <= bound * scale everywhere (absolute; scale = the largest |dv| of the case)."""
    g = got.detach().double().cpu().abs()
    flat = int(g.argmax())
    assert float(g.max()) <= bound * scale, (f"{name}: |value| {float(g.max()):.3e} > {bound:.3e} * {scale:.3e} at flat index {flat} "
                                             f"(token row {flat // g.shape[-1]}, channel {flat % g.shape[-1]})")
    return float(g.max()) / scale


# ----------------------------------------------------------------------------------------------------------------------
# mask mutations (tests/test_attention_probes.py): explicit float64 forward / dv of ONE head that re-evaluates only the mutated rows

class HeadProbe:
    """Count probe of one sequence and one head under the true training mask, float64, with out and raw dv of a mutated mask
    obtained by re-evaluating the softmax of the mutated rows only (dv_n = P^T dO is linear in the rows of P)."""

    def __init__(self, T, P, cls, seed=0):
        self.T, self.P, self.cls = T, P, cls
        self.allowed = O.train_allowed_tokens(T, P)
        x, dO = count_probe(1, 2 * T, P, [cls], self.allowed, seed)
        self.x, self.dO = x, dO
        with torch.no_grad():
            self.q, self.k, self.v = (z[0, 0] for z in prepared_qkv(x.double(), 1, 1, identity_rope(), True))
        self.go = dO.double().reshape(-1, D)
        self.v_raw = x.double()[:, :, 2 * D:].reshape(-1, D)
        p = masked_softmax(self.q, self.k, torch.from_numpy(self.allowed))
        self.p = p
        self.out = p @ self.v
        self.dv_n = p.t() @ self.go
        self.dv = self.raw_dv(self.dv_n)

    def raw_dv(self, dv_n, rows=None):
        """Adjoint of the per-head normalisation of v (autograd through O.normalize); dv_n for all keys, or for the key rows `rows`."""
        vr = (self.v_raw if rows is None else self.v_raw[rows]).clone().requires_grad_(True)
        (g,) = torch.autograd.grad(O.normalize(vr, dim=-1), vr, dv_n)
        return g

    def mutated(self, rows, allowed_rows):
        """rows (r,) query rows, allowed_rows (r, L) their new mask -> (out rows (r, 64), key rows touched, their raw dv)."""
        rows = torch.as_tensor(rows)
        al = torch.as_tensor(allowed_rows)
        p_new = masked_softmax(self.q[rows], self.k, al)
        dp = p_new - self.p[rows]
        keys = dp.abs().sum(0).nonzero()[:, 0]
        dv_n = self.dv_n[keys] + dp[:, keys].t() @ self.go[rows]
        return p_new @ self.v, keys, self.raw_dv(dv_n, keys) if len(keys) else self.dv[:0]

    @staticmethod
    def shift(got, ref):
        """Worst row metric between two sets of rows (r, 64)."""
        if ref.numel() == 0:
            return 0.0
        return float(((got - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-300)).max())
