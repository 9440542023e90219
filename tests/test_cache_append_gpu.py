"""t >= 1 frames appended to a NON-EMPTY evaluation cache: query frame i of the call sees key frame j of the n + t keys iff j <= n + i.

Count probes and random inputs (tests/attention_probes.py) hold every row of the bf16 product path against the float64 reference --
the grid kernels attn_fwd_kernel<1, 1> / <1, 2> with a query frame offset, with and without the rectangular table of
ops.append_mask_table --, then the cache semantics, VideoAttention at every head path and the UNet end to end, chunked against
one-shot.  Measured figures: profiles/cache_append_tests.txt."""
import numpy as np
import pytest
import torch

import attention_probes as AP
from oracle import oniris_oracle as O
from test_attention_probes_gpu import cache_of, dev_rope, line
from test_consistency_gpu import CH, SEED, _bt, _std

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


def append_allowed(n, t, P):
    q = np.arange(t * P)[:, None]
    k = np.arange((n + t) * P)[None, :]
    return (k // P) <= n + (q // P)


def run_eval(x, B, m, cache, update, P, rope):
    from autoregressive_diffusion_amd import ops
    with torch.no_grad():
        out, cache = ops.attention_eval(x.to(DEV, BF16), B, m, dev_rope(rope), cache, update, P)
    torch.cuda.synchronize()
    return out.float().cpu(), cache


def frames_cat(a, b, B):
    """Two packed (B * frames, P, 3C) inputs, sequence-major, joined along the frames of every sequence."""
    return torch.cat([_bt(a, B), _bt(b, B)], dim=1).reshape(-1, *a.shape[1:])


def device_pair(kv, B, m, P):
    """(k, v) (B, m, frames, P, 64) float64 -> the cache pair of the product path: (B, frames * P, m * 64) bf16 on the device."""
    return tuple(z.permute(0, 2, 3, 1, 4).reshape(B, -1, m * 64).to(DEV, BF16) for z in kv)


# ----------------------------------------------------------------------------------------------------------------------
# count probes

APPEND_CASES = [(2, 2, 64, 1),      # table path, aligned
                (1, 2, 64, 2),      # query blocks straddle key blocks
                (3, 3, 64, 1),      # Lq = 192: no table
                (5, 3, 16, 2),      # Lq = 48: partial tiles
                (1, 2, 256, 1),     # table block 256
                (30, 2, 64, 2),     # Lk = 2048: the two-key-stream kernel <1, 2>
                (31, 2, 64, 2)]     # Lk = 2112


@pytest.mark.parametrize("streams", [1, 0], ids=["four-key-streams", "one-key-stream"])
@pytest.mark.parametrize("n,t,P,m", APPEND_CASES)
def test_append_count_probes(n, t, P, m, streams, monkeypatch):
    """Every row of an append puts the same weight on each key frame it may see and none on the others; the frame decoded next,
    against the cache the append left, on each of its frames -- three launches, then the fused qkv launch over the ring's rotated
    image."""
    from autoregressive_diffusion_amd import ops
    monkeypatch.setattr(ops, "DECODE_STREAMS", streams)
    B = 2
    # forward only: the frame class needs no channels for dO, so it serves up to 64 frames (AP.head_classes stops at 32) -- and only
    # it sees a whole key frame dropped or added (the mod-64 class then loses the same share of every channel)
    classes = [("frame", "mod64")[h % 2] for h in range(m)]
    x_old, _ = AP.count_probe(B, n, P, classes)
    x_new, _ = AP.count_probe(B, t, P, classes, frame_offset=[n] * B)
    old = cache_of(x_old, B, m)
    allowed = append_allowed(n, t, P)
    ref, _ = AP.reference(x_new, None, B, m, allowed, AP.identity_rope(), training=False, cache=old)
    rep = {}
    out, cache = run_eval(x_new, B, m, device_pair(old, B, m, P), True, P, AP.identity_rope())
    AP.check_rows("append out", out, ref, m, AP.COUNT_TOL, t, rep)
    assert cache[0].shape[1] == (n + t) * P and cache[1].shape[1] == (n + t) * P
    ring = cache[0]._oniris_ring
    assert ring.n == n + t and ring.kr_state != (ring.n, ring.n + 1)          # no rotated image claimed for the new state
    x1, _ = AP.count_probe(B, 1, P, classes, frame_offset=[n + t] * B)
    ref1, _ = AP.reference(x1, None, B, m, None, AP.identity_rope(), training=False, cache=cache_of(frames_cat(x_old, x_new, B), B, m))
    out3, same = run_eval(x1, B, m, cache, False, P, AP.identity_rope())
    assert same is cache
    AP.check_rows("decode, three launches", out3, ref1, m, AP.COUNT_TOL, 1, rep)
    ring.rotate_committed(dev_rope(AP.identity_rope()))
    assert ring.kr_state == (n + t, n + t + 1)
    out1, cache = run_eval(x1, B, m, cache, True, P, AP.identity_rope())
    AP.check_rows("decode, fused qkv", out1, ref1, m, AP.COUNT_TOL, 1, rep)
    assert cache[0].shape[1] == (n + t + 1) * P and cache[0]._oniris_ring is ring
    line("cache-append", f"n={n} t={t} P={P} heads={m} streams={streams}", rep)


# ----------------------------------------------------------------------------------------------------------------------
# random inputs, real rope: the last t frames of the one-shot prefill over all n + t frames

_random = {}


def random_case(n, t, P, m, B):
    key = (n, t, P, m, B)
    if key not in _random:
        x, dO = AP.random_inputs(B * (n + t), P, m, seed=100 + n)
        allowed = O.infer_allowed_tokens(n + t, P)
        ref, _ = AP.reference(x, None, B, m, allowed, AP.real_rope(), training=False)
        model, _ = AP.model_bf16(x, dO, B, m, allowed, AP.real_rope(), training=False)
        _random[key] = (x, ref, model)
    return _random[key]


@pytest.mark.parametrize("n,t,P,m", [(1, 2, 64, 2), (3, 3, 64, 1), (30, 2, 64, 2)])
def test_append_random_inputs(n, t, P, m):
    """Prefill n frames, append t: every row within RANDOM_BOUND_FACTOR times the worst row of the CPU noise model (bf16 operands,
    P and result) of the same rows -- the bound comes from the model, never from a GPU result."""
    B = 2
    x, ref, model = random_case(n, t, P, m, B)
    last = lambda z: _bt(z, B)[:, n:].reshape(B * t, P, -1)
    noise = max(w for w, _ in AP.worst_rows(last(model), last(ref), m, t))
    bound = AP.RANDOM_BOUND_FACTOR * noise
    xs = _bt(x, B)
    _, cache = run_eval(xs[:, :n].reshape(B * n, P, -1), B, m, None, True, P, AP.real_rope())
    out, cache = run_eval(xs[:, n:].reshape(B * t, P, -1), B, m, cache, True, P, AP.real_rope())
    rep = {"model": noise, "bound": bound}
    try:
        AP.check_rows("append out", out, last(ref), m, bound, t, rep)
    finally:
        line("cache-append-random", f"n={n} t={t} P={P} heads={m}", rep)
    assert cache[0].shape[1] == (n + t) * P


# ----------------------------------------------------------------------------------------------------------------------
# cache semantics

@pytest.mark.selfcheck
def test_append_cache_semantics():
    """update_cache=False hands back the same cache object with its bits; two appends from one cache do not see each other; the pair
    has (n + t) * P rows; one new frame behind an appended chunk gives the bits it gives against a plain copy of that pair (the
    three-launch path of a foreign pair)."""
    B, P, m, n, t = 2, 64, 1, 3, 2
    rope = AP.real_rope()
    g = lambda frames, seed: AP.random_inputs(B * frames, P, m, seed)[0]
    _, c3 = run_eval(g(n, 1), B, m, None, True, P, rope)
    k3, v3 = c3[0].float().clone(), c3[1].float().clone()
    fa, fb = g(t, 2), g(t, 3)
    o_a0, same = run_eval(fa, B, m, c3, False, P, rope)            # (writes the ring's uncommitted slots)
    assert same is c3 and torch.equal(c3[0].float(), k3) and torch.equal(c3[1].float(), v3) and c3[0].shape[1] == n * P
    o_a, ca = run_eval(fa, B, m, c3, True, P, rope)
    assert torch.equal(o_a, o_a0) and ca[0].data_ptr() == c3[0].data_ptr()          # appended in place
    assert ca[0].shape == (B, (n + t) * P, 64 * m) and ca[1].shape == ca[0].shape and ca[0]._oniris_ring.n == n + t
    ka = ca[0].float().clone()
    o_b, cb = run_eval(fb, B, m, c3, True, P, rope)                # a second future from the OLD pair: a ring of its own
    assert cb[0].data_ptr() != ca[0].data_ptr() and cb[0].shape[1] == (n + t) * P
    assert torch.equal(ca[0].float(), ka) and torch.equal(cb[0][:, :n * P].float(), k3)
    assert not torch.equal(cb[0][:, n * P:].float(), ka[:, n * P:])
    o_b2, _ = run_eval(fb, B, m, (k3.to(BF16), v3.to(BF16)), False, P, rope)        # the same chunk against a plain copy of the pair
    assert torch.equal(o_b, o_b2) and not torch.equal(o_b, o_a)
    f1 = g(1, 4)
    o1, c_next = run_eval(f1, B, m, ca, True, P, rope)
    o1_plain, _ = run_eval(f1, B, m, (ca[0].clone(), ca[1].clone()), False, P, rope)
    assert torch.equal(o1, o1_plain) and c_next[0].shape[1] == (n + t + 1) * P


def test_infer_mask_refuses_partial_frames():
    from autoregressive_diffusion_amd import ops
    with pytest.raises(ValueError):
        ops._infer_mask(2, 128, 128 + 32, 64, DEV)
    mode, tabs = ops._infer_mask(2, 128, 256, 64, DEV)
    assert mode == 1 and tabs is not None and tabs[4] == 128 and tabs[1].shape == (1, 2)
    assert ops._infer_mask(3, 192, 384, 64, DEV) == (1, None)


# ----------------------------------------------------------------------------------------------------------------------
# modules: chunked against one-shot

@pytest.mark.selfcheck
@pytest.mark.parametrize("hc", [16, 48, 64, 128], ids=lambda c: f"head{c}")
def test_video_attention_chunked_vs_one_shot(hc):
    """8 frames of 16x16 in one call against 5 frames, then 2, then 1 through the cache: padded heads (16, 48), the KV ring (64) and
    the wide-head path (128).  Bound of test_video_attention_cached_vs_non_cached, on every frame."""
    from edm2.attention import VideoAttention
    torch.manual_seed(SEED)
    att = VideoAttention(channels=4 * hc, num_heads=4).to(DEV).eval()
    B, T, RES = 2, 8, 16
    x = torch.randn(B, T, att.channels, RES, RES, device=DEV)
    flat = lambda z: z.reshape(-1, *z.shape[2:])
    with torch.no_grad():
        y_full, _ = att(flat(x), B)
        y0, cache = att(flat(x[:, :5]), B, update_cache=True)
        y1, cache = att(flat(x[:, 5:7]), B, cache, update_cache=True)
        y2, cache = att(flat(x[:, 7:]), B, cache, update_cache=True)
    y_full = _bt(y_full, B)
    got = torch.cat([_bt(y0, B), _bt(y1, B), _bt(y2, B)], dim=1)
    s = y_full.std().item()
    worst = max(_std(y_full[:, f], got[:, f]) for f in range(T))
    print(f"PROBE cache-append-module head={hc} worst_frame_std={worst:.3e} std_y={s:.3e}")
    assert worst <= 1e-2 * s
    frames = cache[0].shape[2] if cache[0].dim() == 5 else cache[0].shape[1] // (RES * RES)      # (wide heads keep (b, m, frames, P, d))
    assert frames == T


# ----------------------------------------------------------------------------------------------------------------------
# net: chunks of 2 + 3 + 1 against one evaluation of 6 frames, then a sampled frame from either cache

def small_net():
    from edm2.networks_edm2 import UNet, Precond
    torch.manual_seed(SEED)
    unet = UNet(img_resolution=32, img_channels=CH, label_dim=0, model_channels=32, channel_mult=[1, 2, 2, 4],
                channel_mult_noise=None, channel_mult_emb=None, num_blocks=3, video_attn_resolutions=[16, 8]).to(DEV)
    with torch.no_grad():                  # (as tests/test_consistency_gpu.py: give the output a scale and the temporal paths a weight)
        unet.out_gain.fill_(1.0)
        for name, p in unet.named_parameters():
            if name.endswith("gating.max_gating"):
                p.fill_(1.0)
            elif name.endswith("gating.min_gating"):
                p.fill_(-1.0)
    return Precond(unet, use_fp16=True, sigma_data=0.5).to(DEV).eval()


def conv_caches(cache, path=()):
    """[(path, activation pair, frame counter)] of every gated conv's cache entry, in a fixed order."""
    found = []
    for k in sorted(cache, key=str):
        v = cache[k]
        if isinstance(v, dict):
            if "activations" in v:
                found.append((path + (k,), v["activations"], v.get("n_context_frames")))
            found += conv_caches(v, path + (k,))
    return found


@pytest.mark.selfcheck
def test_net_chunked_vs_one_shot():
    from autoregressive_diffusion_amd import ops
    from edm2.sampler import edm_sampler_with_mse
    net = small_net()
    B, T = 2, 6
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, T, CH, 32, 32, generator=g).to(DEV)
    sigma = (torch.rand(B, T, generator=g) * 0.5 + 0.05).to(DEV)
    with torch.no_grad():
        y_full, c_full = net(x, sigma, None, update_cache=True)
        cache, got = None, []
        for a, b in ((0, 2), (2, 5), (5, 6)):
            y, cache = net(x[:, a:b].contiguous(), sigma[:, a:b].contiguous(), None, cache=cache, update_cache=True)
            got.append(y)
    got = torch.cat(got, dim=1)
    s = y_full.std().item()
    worst = max(_std(y_full[:, f], got[:, f]) for f in range(T))
    print(f"PROBE cache-append-net worst_frame_std={worst:.3e} std_y={s:.3e}")
    assert s > 0 and worst <= 2e-2 * s
    assert cache["n_context_frames"] == c_full["n_context_frames"] == T
    one, chunked = conv_caches(c_full), conv_caches(cache)
    assert len(one) == len(chunked) > 0
    for (pa, a, na), (pb, b, nb) in zip(one, chunked):
        assert pa == pb and na == nb == T, (pa, pb, na, nb)
        assert _std(a, b) <= 2e-2 * max(a.float().std().item(), 1e-6), pa
    # the sampler picks the appended rings up: room for the next frame in the SAME ring, the rotated image ready for the fused launch
    rings = [v["attn"][0]._oniris_ring for v in cache.values() if isinstance(v, dict) and isinstance(v.get("attn"), tuple)]
    assert rings and all(r.n == T for r in rings)
    net.unet.prewarm_eval(cache)
    now = [v["attn"][0]._oniris_ring for v in cache.values() if isinstance(v, dict) and isinstance(v.get("attn"), tuple)]
    assert all(a is b and a.kr_state == (T, T + 1) for a, b in zip(rings, now))
    noise = torch.randn(B, 1, CH, 32, 32, generator=g).to(DEV)
    frames = []
    with torch.no_grad():
        for c in (c_full, cache):
            xf, _, _, c = edm_sampler_with_mse(net, c, num_steps=4, sigma_min=0.01, sigma_max=80, rho=2, noise=noise)
            frames.append(xf.clone())
            assert c["n_context_frames"] == T + 1
    assert torch.isfinite(frames[0]).all()
    assert _std(frames[0], frames[1]) <= 2e-2 * frames[0].std().item()
