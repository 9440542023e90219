"""A bounded context window (UNet.set_context_window, the trailing `window` of the eval attention ops): the cache keeps the last W
frames, a call still attends to everything cached plus its own frames.  The yardstick is the same sequence of calls on a cache
whose every (K, V) pair is sliced by hand to its last W frames before each call -- the reference's behaviour --, which drops the KV
ring every time; the windowed ring must give the same numbers from one fixed storage of 2 W frames."""
import copy
import pytest
import torch

import attention_probes as AP
import test_model_gpu as M
from test_attention_probes_gpu import dev_rope
from test_consistency_gpu import SEED, TIGHT, _bt, _std

pytestmark = [pytest.mark.gpu, pytest.mark.selfcheck]      # (the HIP path against itself: not counted as oracle coverage)
DEV = "cuda"
BF16 = torch.bfloat16


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30)).item()


def sliced(kv, W, P):
    return None if kv is None else (kv[0][:, -W * P:], kv[1][:, -W * P:])


@pytest.mark.parametrize("fused_knob", [0, 1], ids=["unfused-qkv", "default"])
@pytest.mark.parametrize("W", [2, 3])
def test_windowed_ring_matches_hand_sliced_pair(W, fused_knob, monkeypatch):
    """Prefill 1 frame, 2W + 3 single-frame commits (past the fill at frame W and at least one move to the front), one append of
    t = 2 with n + t > W.  The launches are the same on both sides: outputs and the kept K, V are equal bit for bit; the ring's
    storage holds 2W frames and stays where it is."""
    from autoregressive_diffusion_amd import ops
    monkeypatch.setattr(ops, "FUSED_QKV_EVAL", fused_knob)
    B, P, m = 2, 64, 1
    rb = dev_rope(AP.real_rope())
    chunks = [1] + [1] * (2 * W + 3) + [2]
    cw, ch, ptrs, worst, moves = None, None, [], 0.0, 0
    with torch.no_grad():
        for i, t in enumerate(chunks):
            x = AP.random_inputs(B * t, P, m, seed=50 + i)[0].to(DEV, BF16)
            ow, cw = ops.attention_eval(x, B, m, rb, cw, True, P, window=W)
            oh, ch = ops.attention_eval(x, B, m, rb, sliced(ch, W, P), True, P)
            kept = min(W, sum(chunks[:i + 1]))
            assert cw[0].shape == (B, kept * P, 64 * m) and cw[1].shape == cw[0].shape
            worst = max(worst, _std(ow, oh))
            assert torch.equal(ow, oh), (i, t)
            assert torch.equal(cw[0], ch[0][:, -W * P:]) and torch.equal(cw[1], ch[1][:, -W * P:]), (i, t)
            ring = cw[0]._oniris_ring
            if t == 1:
                ptrs.append((ring.K.data_ptr(), ring.V.data_ptr(), ring.cap))
                moves = max(moves, ring.moves)
    assert worst <= TIGHT
    assert len(set(ptrs[-(W + 2):])) == 1 and ptrs[-1][2] == 2 * W, ptrs
    assert ring.window == W and moves >= 1                                     # the live frames went to the front at least once
    with pytest.raises(ValueError):
        ops.attention_eval(x, B, m, rb, None, True, P, window=0)


@pytest.mark.parametrize("W", [2, 3])
def test_windowed_ring_fused_decode(W):
    """The sampler's way to the decode kernel on a windowed ring: the live keys rotated once (KVRing.rotate_committed), then the
    fused qkv launch writes behind them -- wherever the window starts in the storage --, against the three launches on the
    hand-sliced pair.  Bound: 2e-3 relative, the project's bound for fused against three launches
    (test_decode_attention_at_rollout_depth_vs_oracle)."""
    from autoregressive_diffusion_amd import ops
    B, P, m = 2, 64, 2
    rb = dev_rope(AP.real_rope())
    cw, ch, worst, starts = None, None, 0.0, set()
    with torch.no_grad():
        for i in range(2 * W + 4):
            x = AP.random_inputs(B, P, m, seed=80 + i)[0].to(DEV, BF16)
            if cw is not None:
                ring = cw[0]._oniris_ring
                ring.rotate_committed(rb)
                assert ring.kr_state == (ring.n, ring.n + 1)
                starts.add(ring.start)
            ow, cw = ops.attention_eval(x, B, m, rb, cw, True, P, window=W)
            oh, ch = ops.attention_eval(x, B, m, rb, sliced(ch, W, P), True, P)
            worst = max(worst, rel(ow, oh))
            assert rel(cw[0], ch[0][:, -W * P:]) < 2e-3 and rel(cw[1], ch[1][:, -W * P:]) < 2e-3, i
    print(f"PROBE context-window-fused W={W} worst_rel={worst:.3e} ring_starts={sorted(starts)}")
    assert len(starts) > 1                       # the window sat at more than one place in the storage
    assert worst < 2e-3


@pytest.mark.parametrize("hc", [16, 64, 128], ids=lambda c: f"head{c}")
def test_video_attention_window_matches_hand_slicing(hc):
    """Padded heads (16), the KV ring (64) and wide heads (128) through the module."""
    from edm2.attention import VideoAttention
    torch.manual_seed(SEED)
    W, B, RES = 2, 2, 8
    att = VideoAttention(channels=4 * hc, num_heads=4).to(DEV).eval()
    twin = copy.deepcopy(att)
    att.context_window = W
    P = RES * RES
    cut = (lambda z: z[:, :, -W:]) if hc > 64 else (lambda z: z[:, -W * P:])      # (wide heads keep (b, m, frames, P, d))
    cw, ch = None, None
    with torch.no_grad():
        for i, t in enumerate([1, 1, 1, 1, 2, 1, 1]):
            x = torch.randn(B * t, att.channels, RES, RES, device=DEV)
            yw, cw = att(x, B, cw, update_cache=True)
            yh, ch = twin(x, B, None if ch is None else (cut(ch[0]), cut(ch[1])), update_cache=True)
            assert _std(yw, yh) <= TIGHT * max(1.0, yh.std().item()), (i, t)
            kw, kh = cw[0], cut(ch[0])
            assert kw.shape == kh.shape and torch.equal(kw, kh), (i, t)


def test_video_attention_window_fp32_mode():
    """The fp32 verification path (Precond(use_fp16=False) / force_fp32=True) keeps (b, m, frames, P, d) and slices its frames."""
    from autoregressive_diffusion_amd import fp32
    from edm2.attention import VideoAttention
    torch.manual_seed(SEED)
    W, B, RES = 2, 2, 8
    att = VideoAttention(channels=128, num_heads=2).to(DEV).eval()
    twin = copy.deepcopy(att)
    att.context_window = W
    cut = lambda z: z[:, :, -W:]
    cw, ch = None, None
    with torch.no_grad(), fp32.fp32_arithmetic():
        for i, t in enumerate([1, 1, 2, 1]):
            x = torch.randn(B * t, att.channels, RES, RES, device=DEV)
            yw, cw = att(x, B, cw, update_cache=True)
            yh, ch = twin(x, B, None if ch is None else (cut(ch[0]), cut(ch[1])), update_cache=True)
            assert torch.equal(yw, yh) and cw[0].shape[2] == min(W, sum([1, 1, 2, 1][:i + 1])) and torch.equal(cw[0], cut(ch[0])), (i, t)


# ----------------------------------------------------------------------------------------------------------------------
# sampler

W_S, CTX, GEN, STEPS, B_S = 3, 2, 8, 4, 1
_rollouts = {}


def hand_slice(cache, W):
    for v in cache.values():
        if isinstance(v, dict) and isinstance(v.get("attn"), tuple):
            P = 64                                                     # 8x8 tokens per frame at every VideoAttention of SMALL_CFG
            v["attn"] = sliced(v["attn"], W, P)


def rollout(kind, guidance=1):
    """kind: 'window' (set_context_window(W)), 'hand' (no window, pairs sliced before every frame), 'eager' ('window' without the
    graph), 'none' (set_context_window(None)), 'never'."""
    key = (kind, guidance)
    if key in _rollouts:
        return _rollouts[key]
    import edm2.sampler as S
    net = M.build_precond(M.SMALL_CFG, 91, 0.5).eval()
    if kind in ("window", "eager"):
        assert net.set_context_window(W_S) is net
    elif kind == "none":
        net.set_context_window(W_S).set_context_window(None)
    g = torch.Generator().manual_seed(11)
    ctx = torch.randn(B_S, CTX, 4, 32, 32, generator=g).to(DEV)
    labels = torch.randint(0, 4, (B_S, CTX), generator=g).to(DEV)
    old = S.SAMPLER_GRAPH
    S.SAMPLER_GRAPH = 0 if kind == "eager" else 1
    frames = []
    try:
        with torch.no_grad():
            _, cache = net(ctx, torch.ones(B_S, CTX, device=DEV) * 0.05, labels, update_cache=True)
            for f in range(GEN):
                noise = torch.randn(B_S, 1, 4, 32, 32, generator=g).to(DEV)
                if kind == "hand":
                    hand_slice(cache, W_S)
                x, _, _, cache = S.edm_sampler_with_mse(net, cache, conditioning=torch.full((B_S, 1), f % 4, device=DEV),
                                                        num_steps=STEPS, sigma_min=0.01, sigma_max=80, rho=2, noise=noise,
                                                        guidance=guidance)
                frames.append(x.clone())
    finally:
        S.SAMPLER_GRAPH = old
    kv = cache[("enc", "8x8_block0")]["attn"]
    torch.cuda.synchronize()
    _rollouts[key] = (torch.cat(frames, dim=1), kv[0].float().clone(), cache["n_context_frames"], getattr(kv[0], "_oniris_ring", None))
    return _rollouts[key]


def test_sampler_window_matches_hand_slicing():
    fw, kw, nw, ring = rollout("window")
    fh, kh, nh, _ = rollout("hand")
    assert torch.isfinite(fw).all() and nw == nh == CTX + GEN                 # the gates keep counting
    assert kw.shape[1] == W_S * 64 and ring is not None and ring.window == W_S and ring.cap == 2 * W_S and ring.moves >= 1
    worst = max(_std(fw[:, f], fh[:, f]) for f in range(GEN))
    print(f"PROBE context-window-sampler worst_frame_std={worst:.3e} std_x={fh.std().item():.3e}")
    assert worst <= TIGHT * max(1.0, fh.std().item())
    assert _std(kw, kh[:, -W_S * 64:]) <= TIGHT


def test_sampler_window_graph_matches_eager():
    fw, kw, nw, _ = rollout("window")
    fe, ke, ne, _ = rollout("eager")
    assert nw == ne and rel(fw, fe) < 1e-5 and rel(kw, ke) < 1e-5             # as test_sampler_graph_replay_matches_eager asserts it


def test_sampler_window_none_is_unbounded():
    fa, ka, na, _ = rollout("none")
    fb, kb, nb, _ = rollout("never")
    assert na == nb and torch.equal(fa, fb) and torch.equal(ka, kb) and ka.shape[1] == (CTX + GEN) * 64


def test_sampler_window_guided():
    fw, kw, _, ring = rollout("window", guidance=2)
    fh, kh, _, _ = rollout("hand", guidance=2)
    assert torch.isfinite(fw).all() and kw.shape[1] == W_S * 64 and ring.cap == 2 * W_S
    worst = max(_std(fw[:, f], fh[:, f]) for f in range(GEN))
    print(f"PROBE context-window-guided worst_frame_std={worst:.3e} std_x={fh.std().item():.3e}")
    assert worst <= TIGHT * max(1.0, fh.std().item())


def test_context_window_is_a_plain_attribute():
    from edm2.attention import VideoAttention
    net = M.build_precond(M.SMALL_CFG, 91, 0.5)
    keys = list(net.state_dict().keys())
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            net.set_context_window(bad)
    net.set_context_window(5)
    layers = [m for m in net.modules() if isinstance(m, VideoAttention)]
    assert layers and all(m.context_window == 5 for m in layers) and net.unet.context_window == 5
    twin = copy.deepcopy(net)
    assert twin.unet.context_window == 5 and all(m.context_window == 5 for m in twin.modules() if isinstance(m, VideoAttention))
    assert list(net.state_dict().keys()) == keys and "context_window" not in net.unet.kwargs
    assert net.unet.set_context_window(None) is net.unet and all(m.context_window is None for m in layers)
