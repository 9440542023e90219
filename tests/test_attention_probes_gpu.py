"""The attention kernels row by row: count probes and random inputs (tests/attention_probes.py) against the float64 reference.

Count probes (constant q = k, identity rope, one-hot v and dO): every row of `out` and of the v part of dqkv within COUNT_TOL = 2^-6
of the reference -- tests/test_attention_probes.py shows that one wrong (query, key) pair moves a row of `out`, and a wrong group
of pairs a row of dv, by at least three times that --, and the q and k parts of dqkv, zero in the reference, within 2^-6 of the
largest |dv|.  Random inputs (real rope tables): every row of out, dq, dk, dv within RANDOM_BOUND_FACTOR = 4 times the worst row
of the CPU noise model (AP.model_bf16: float32 with bf16 P, operands and results) against the same float64 reference; the bound
is computed here from the model, never from a GPU result.  Measured figures: profiles/attention_probes.txt."""
import numpy as np
import pytest
import torch

import attention_probes as AP
from oracle import oniris_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def dev_rope(rope):
    return tuple(z.to(DEV) for z in rope)


def run_train(x, dO, kind, B, T, m, rope):
    from autoregressive_diffusion_amd import ops
    xg = x.detach().to(DEV, BF16).requires_grad_(True)
    out = ops.attention_train(xg, kind, B, T, m, None if rope is None else dev_rope(rope))
    out.backward(dO.to(DEV, BF16))
    torch.cuda.synchronize()
    return out.detach().float().cpu(), xg.grad.float().cpu()


def line(tag, case, figures):
    print(f"PROBE {tag} {case} " + " ".join(f"{k}={v:.3e}" for k, v in figures.items()))


def random_bounds(model, ref, heads):
    """4 x the worst row of the CPU noise model, per tensor (over all heads)."""
    mo, mg = model
    ro, rg = ref
    worst = {"out": max(w for w, _ in AP.worst_rows(mo, ro, heads))}
    for name in ("dq", "dk", "dv"):
        worst[name] = max(w for w, _ in AP.worst_rows(AP.split_dqkv(mg)[name], AP.split_dqkv(rg)[name], heads))
    return worst, {k: AP.RANDOM_BOUND_FACTOR * v for k, v in worst.items()}


def check_random(tag, case, got, ref, model, heads, frames_per_seq):
    noise, bound = random_bounds(model, ref, heads)
    rep = {}
    errs = []
    parts = [("out", got[0], ref[0])] + [(n, AP.split_dqkv(got[1])[n], AP.split_dqkv(ref[1])[n]) for n in ("dq", "dk", "dv")]
    for name, g, r in parts:
        try:
            AP.check_rows(name, g, r, heads, bound[name], frames_per_seq, rep)
        except AssertionError as e:
            errs.append(str(e))
    line(tag, case, {**rep, **{f"model_{k}": v for k, v in noise.items()}})
    assert not errs, f"{case}: " + " | ".join(errs)


def check_count(tag, case, got, ref, heads, frames_per_seq):
    rep = {}
    errs = []
    g, r = AP.split_dqkv(got[1]), AP.split_dqkv(ref[1])
    scale = float(r["dv"].abs().max())
    for name, a, b in (("out", got[0], ref[0]), ("dv", g["dv"], r["dv"])):
        try:
            AP.check_rows(name, a, b, heads, AP.COUNT_TOL, frames_per_seq, rep)
        except AssertionError as e:
            errs.append(str(e))
    for name in ("dq", "dk"):
        try:
            rep[name + "_abs"] = AP.check_zero(name, g[name], scale)
        except AssertionError as e:
            errs.append(str(e))
    line(tag, case, rep)
    assert not errs, f"{case}: " + " | ".join(errs)


# ----------------------------------------------------------------------------------------------------------------------
# VideoAttention, training

# (ATTN_PERSISTENT, DKV_ITEM_KEYS, ATTN_DKV_CHUNKS, ATTN_DQ_PERSISTENT, ATTN_DKV_PERSISTENT); None: leave the default.
# The cross of the five knobs, without the combinations ops.py maps to the same launches: the item size only exists in the
# persistent dK/dV kernel, the chunks only in the grid dK/dV kernel, and the persistent dQ kernel only runs next to the
# persistent dK/dV kernel (ops._attn_core_bwd).
DEFAULTS = (1, None, None, 1, 1)
GRID = (0, 0, 1, 1, 1)
CROSS = ([(1, keys, 1, dq, 1) for keys in (0, 128) for dq in (1, 0)]        # persistent forward, dK/dV; dQ persistent / grid
         + [(1, 0, chunks, 1, 0) for chunks in (1, 3)]                      # persistent forward, grid dQ and dK/dV
         + [(0, 0, chunks, 1, 1) for chunks in (1, 3)])                     # grid kernels throughout
VIDEO_CASES = ([(shape, knobs) for shape in [(1, 8, 4, 2), (1, 16, 8, 2)] for knobs in CROSS]
               + [(shape, knobs) for shape in [(1, 4, 8, 2), (1, 32, 4, 2), (1, 2, 16, 2), (3, 4, 8, 4)] for knobs in (DEFAULTS, GRID)])


def set_video_knobs(monkeypatch, knobs):
    from autoregressive_diffusion_amd import ops
    persistent, keys, chunks, dq, dkv = knobs
    monkeypatch.setattr(ops, "ATTN_PERSISTENT", persistent)
    monkeypatch.setattr(ops, "ATTN_DQ_PERSISTENT", dq)
    monkeypatch.setattr(ops, "ATTN_DKV_PERSISTENT", dkv)
    if keys is not None:
        monkeypatch.setattr(ops, "DKV_ITEM_KEYS", keys)
    if chunks is not None:
        monkeypatch.setattr(ops, "ATTN_DKV_CHUNKS", chunks)
        monkeypatch.setattr(ops, "ATTN_DKV_MIN_L", 128)


def video_count_case(B, T, H, m):
    P = H * H
    allowed = O.train_allowed_tokens(T, P)
    classes = AP.head_classes(m, 2 * T)
    x, dO = AP.count_probe(B, 2 * T, P, classes, allowed)
    ref = AP.reference(x[:2 * T], dO[:2 * T], 1, m, allowed, AP.identity_rope())          # every sequence carries the same probe
    return x, dO, tuple(z.repeat(B, 1, 1) for z in ref)


def video_random_case(B, T, H, m):
    P = H * H
    allowed = O.train_allowed_tokens(T, P)
    x, dO = AP.random_inputs(B * 2 * T, P, m, seed=5 + T + H)
    return x, dO, AP.reference(x, dO, B, m, allowed, AP.real_rope()), AP.model_bf16(x, dO, B, m, allowed, AP.real_rope())


@pytest.mark.parametrize("shape,knobs", VIDEO_CASES)
def test_video_attention_count_probes(shape, knobs, monkeypatch):
    B, T, H, m = shape
    set_video_knobs(monkeypatch, knobs)
    x, dO, ref = cached(("vc",) + shape, lambda: video_count_case(*shape))
    got = run_train(x, dO, "video", B, T, m, AP.identity_rope())
    check_count("video-count", f"{shape} knobs={knobs}", got, ref, m, 2 * T)


@pytest.mark.parametrize("shape,knobs", VIDEO_CASES)
def test_video_attention_random_rows(shape, knobs, monkeypatch):
    B, T, H, m = shape
    set_video_knobs(monkeypatch, knobs)
    x, dO, ref, model = cached(("vr",) + shape, lambda: video_random_case(*shape))
    got = run_train(x, dO, "video", B, T, m, AP.real_rope())
    check_random("video-random", f"{shape} knobs={knobs}", got, ref, model, m, 2 * T)


# ----------------------------------------------------------------------------------------------------------------------
# FrameAttention, training

# variant (test_frame_attention_core_train): 3 = the two launches that read the raw qkv, 1 = qkv_norm passes around the frame forward
# + one-launch backward, 2 = ... around the frame forward, frame dQ and grid dK / dV kernels, 0 = grid kernels; "ws": the persistent
# work lists (FRAME_WS = 1, frames of 128 * 2^k tokens: the variant plays no part there).  16-token frames: grid kernels whatever
# the variant.
FRAME_CASES = ([((N, P, m), v) for (N, P, m) in [(5, 64, 2), (13, 64, 4), (5, 128, 1), (6, 128, 2), (3, 256, 2), (16, 256, 2)] for v in (3, 1, 2, 0)]
               + [((N, P, m), "ws") for (N, P, m) in [(5, 128, 1), (6, 128, 2), (3, 256, 2), (16, 256, 2)]]
               + [((3, 16, 1), 0)])


def set_frame_knobs(monkeypatch, variant):
    from autoregressive_diffusion_amd import ops
    ws = variant == "ws"
    v = 3 if ws else variant
    monkeypatch.setattr(ops, "FRAME_WS", int(ws))
    monkeypatch.setattr(ops, "FRAME_KERNEL", min(v, 1))
    monkeypatch.setattr(ops, "FRAME_BWD_FUSED", int(v in (1, 3)))
    monkeypatch.setattr(ops, "FRAME_QKV_FUSED", int(v == 3))


def frame_count_case(N, P, m):
    x, dO = AP.count_probe(N, 1, P, ["frame"] * m, np.ones((P, P), dtype=bool), frame_offset=np.arange(N))
    return x, dO, AP.reference(x, dO, N, m, None)


def frame_random_case(N, P, m):
    x, dO = AP.random_inputs(N, P, m, seed=N * P + m)
    return x, dO, AP.reference(x, dO, N, m, None), AP.model_bf16(x, dO, N, m, None)


@pytest.mark.parametrize("case,variant", FRAME_CASES)
def test_frame_attention_count_probes(case, variant, monkeypatch):
    """Every frame has its own class: a row of `out` holds nothing outside its frame's channel, a row of dv nothing outside its
    frame's gradient channel -- weight anywhere else is leakage from another frame of the super-block / work list."""
    N, P, m = case
    set_frame_knobs(monkeypatch, variant)
    x, dO, ref = cached(("fc",) + case, lambda: frame_count_case(*case))
    got = run_train(x, dO, "frame", N, 1, m, None)
    check_count("frame-count", f"{case} variant={variant}", got, ref, m, 1)
    # (stated on its own: the reference rows are one-hot)
    for name, g, r in (("out", got[0], ref[0]), ("dv", AP.split_dqkv(got[1])["dv"], AP.split_dqkv(ref[1])["dv"])):
        r4, g4 = r.reshape(N, P, m, 64), g.double().reshape(N, P, m, 64)
        hot = r4.abs().amax(-1, keepdim=True)
        assert ((r4.abs() > 1e-3 * hot).sum(-1) == 1).all()
        leak = (g4.abs() * (r4.abs() <= 1e-3 * hot)).amax(-1) / hot[..., 0]
        assert leak.max() <= AP.COUNT_TOL, f"{name}: weight {float(leak.max()):.3e} of a row outside its own frame's channel"


@pytest.mark.parametrize("case,variant", FRAME_CASES)
def test_frame_attention_random_rows(case, variant, monkeypatch):
    N, P, m = case
    set_frame_knobs(monkeypatch, variant)
    x, dO, ref, model = cached(("fr",) + case, lambda: frame_random_case(*case))
    got = run_train(x, dO, "frame", N, 1, m, None)
    check_random("frame-random", f"{case} variant={variant}", got, ref, model, m, 1)


# ----------------------------------------------------------------------------------------------------------------------
# evaluation: prefill and decode, count probes

def run_eval(x, B, m, cache, update, P):
    from autoregressive_diffusion_amd import ops
    with torch.no_grad():
        out, cache = ops.attention_eval(x.to(DEV, BF16), B, m, dev_rope(AP.identity_rope()), cache, update, P)
    torch.cuda.synchronize()
    return out.float().cpu(), cache


def cache_of(x, B, m):
    """Normalised k, v (B, m, frames, P, 64) of packed x in float64: what the reference keeps as the cache.  k stays unrounded:
    every key carries the same vector, and rounding the cached copies alone would make the REFERENCE's softmax non-uniform."""
    _, k, v = AP.prepared_qkv(x.double(), B, m, None, False)
    P = x.shape[1]
    return tuple(z.reshape(B, m, -1, P, 64) for z in (k, v))


@pytest.mark.parametrize("streams", [1, 0], ids=["four-key-streams", "one-key-stream"])
@pytest.mark.parametrize("cls", ["frame", "mod64"])
@pytest.mark.parametrize("t0", [4, 5, 1])
def test_attention_eval_prefill_count_probes(t0, cls, streams, monkeypatch):
    """Prefill under the frame-causal mask (mask_mode 1): table path (t0 = 4), dense fall-back (t0 * P not a multiple of 128),
    score_mod path (one frame), then one decoded frame against the cache the prefill left."""
    from autoregressive_diffusion_amd import ops
    monkeypatch.setattr(ops, "DECODE_STREAMS", streams)
    B, H, m = 2, 8, 1
    P = H * H
    x0, _ = AP.count_probe(B, t0, P, [cls])
    allowed = None if t0 == 1 else O.infer_allowed_tokens(t0, P)
    ref0, _ = AP.reference(x0, None, B, m, allowed, AP.identity_rope(), training=False)
    out0, cache = run_eval(x0, B, m, None, True, P)
    rep = {}
    AP.check_rows("prefill out", out0, ref0, m, AP.COUNT_TOL, t0, rep)
    x1, _ = AP.count_probe(B, 1, P, [cls], frame_offset=[t0] * B)
    ref1, _ = AP.reference(x1, None, B, m, None, AP.identity_rope(), training=False, cache=cache_of(x0, B, m))
    out1, cache = run_eval(x1, B, m, cache, True, P)
    AP.check_rows("decode out", out1, ref1, m, AP.COUNT_TOL, 1, rep)
    assert cache[0].shape[1] == (t0 + 1) * P
    line("eval-prefill", f"t0={t0} cls={cls} streams={streams}", rep)


@pytest.mark.parametrize("streams", [1, 0], ids=["four-key-streams", "one-key-stream"])
@pytest.mark.parametrize("B,H,m,n_old", [(1, 8, 2, 8), (1, 8, 2, 31), (1, 8, 2, 36), (2, 4, 2, 5), (2, 4, 2, 6)])
def test_decode_count_probes(B, H, m, n_old, streams, monkeypatch):
    """One new frame against a ring of n_old frames, every key frame with a class of its own: each row of `out` must put the
    same weight 1 / (n_old + 1) on every frame, the new one included.  31 cached frames of 64 tokens + the new one = 2048 keys, the
    first size on the split-KV path; 36: 2368 keys, tiles dealt unevenly over the splits; 16-token frames: 5 and 6 cached frames
    leave a partial 64-key tail tile.  Both ways to the decode kernel: three launches, and the fused qkv launch over the ring's
    rotated image (KVRing.rotate_committed)."""
    from autoregressive_diffusion_amd import ops
    monkeypatch.setattr(ops, "DECODE_STREAMS", streams)
    P, C = H * H, 64 * m
    classes = ["frame"] * m
    x_old, _ = AP.count_probe(B, n_old, P, classes)
    k_old, v_old = cache_of(x_old, B, m)
    v_old = AP.bfr(v_old.float()).double()
    ring = ops.KVRing(B, P, C, n_old + 2, DEV)
    to_ring = lambda z: z.permute(0, 2, 3, 1, 4).reshape(B, n_old * P, C).to(DEV, BF16)
    ring.K[:, :n_old * P], ring.V[:, :n_old * P], ring.n = to_ring(k_old), to_ring(v_old), n_old
    cache = ring.views()
    x1, _ = AP.count_probe(B, 1, P, classes, frame_offset=[n_old] * B)
    ref, _ = AP.reference(x1, None, B, m, None, AP.identity_rope(), training=False, cache=(k_old, v_old))
    # the reference itself: equal weight on each of the n_old + 1 frames
    r4 = ref.reshape(B, P, m, 64)
    assert (r4[..., :n_old + 1] / r4[..., :1] - 1).abs().max() < 2e-3 and r4[..., n_old + 1:].abs().max() == 0
    rep = {}
    out3, same = run_eval(x1, B, m, cache, False, P)
    assert same is cache
    AP.check_rows("three launches", out3, ref, m, AP.COUNT_TOL, 1, rep)
    ring.rotate_committed(dev_rope(AP.identity_rope()))
    assert ring.kr_state == (n_old, n_old + 1)
    out1, cache = run_eval(x1, B, m, cache, True, P)
    AP.check_rows("fused qkv", out1, ref, m, AP.COUNT_TOL, 1, rep)
    assert cache[0].shape[1] == (n_old + 1) * P
    line("decode", f"B={B} P={P} m={m} cached={n_old} streams={streams}", rep)
