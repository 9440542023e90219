"""edm_sampler_with_mse with S_churn > 0 and / or target= on the graph-replay frame loop (edm2/sampler.py::_fused_frame): every
evaluation a replay, the churn injection and the MSE partials inside the update launches (oniris_sampler_step), the means read with one
copy after the last step.  SMALL_CFG, the inputs of fixture G9b, num_steps=4, sigma_min=0.01, sigma_max=80, rho=2.

  1. against the fixture (the reference's own outputs): frames rel L2 < 5e-2, MSE lists rtol 5e-2, cache counters -- the bounds
     tests/test_model_gpu.py::test_g9b_sampler_side_branches holds the tensor-expression loop to;
  2. against ONIRIS_SAMPLER_FUSED=0 in the same process on the same noise: frames rel L2 < 1e-5 (the bound of
     test_sampler_graph_replay_matches_eager), MSE lists rtol 1e-4: a frame difference of 1e-5 moves an MSE by 2 * 1e-5 * |x| / |x - target|,
     that ratio is about 1 on these inputs (mse 88..1300 at |x|^2 100..1600; mse_pred 0.7 at |x_pred|^2 1), plus 2^-17 for the
     fp32 mean: roughly threefold room;
  3. the generator sees the same draws in the same order on both loops;
  4. no .item() anywhere in a probed frame; 5. a probe leaves the cache as it found it; 6. a churned frame is ONE call of the net.
Every figure is printed as `CHURN <case> <figure> <value / bound>` (pytest -s); profiles/sampler_churn_target_tests.txt."""
import numpy as np
import pytest
import torch

from test_model_gpu import DEV, SMALL_CFG, T, build_precond, load, rel

pytestmark = pytest.mark.gpu
KW = dict(num_steps=4, sigma_min=0.01, sigma_max=80, rho=2)
_state = {}


def _fork(c):
    return {k: _fork(v) for k, v in c.items()} if isinstance(c, dict) else c      # fresh dicts, shared tensors


def _setup():
    """The net, the prefill cache and the inputs of fixture G9b, built once and never modified (tests work on forks)."""
    if not _state:
        z = load("g9b_sampler_branches")
        net = build_precond(SMALL_CFG, int(z["seed"]), 0.5).eval()
        with torch.no_grad():
            _, cache0 = net(T(z["ctx"]).to(DEV), torch.ones(1, 4, device=DEV) * 0.05, T(z["ctx_labels"]).to(DEV), update_cache=True)
        _state.update(z=z, net=net, cache0=cache0, noise=T(z["noise"]).to(DEV), churn_noise=T(z["churn_noise"]).to(DEV),
                      target=T(z["target"]).to(DEV), cond=torch.full((1, 1), 2, device=DEV))
    return _state


def _kv_len(cache):
    return cache[("enc", "8x8_block0")]["attn"][0].shape[1]


def _sample(fused, cache=None, given_noise=True, **kw):
    import edm2.sampler as S
    s = _setup()
    old = S.FUSED_FRAME
    S.FUSED_FRAME = fused
    try:
        with torch.no_grad():
            extra = dict(noise=s["noise"], churn_noise=s["churn_noise"]) if given_noise else {}
            return S.edm_sampler_with_mse(s["net"], _fork(s["cache0"]) if cache is None else cache, conditioning=s["cond"], **KW, **extra, **kw)
    finally:
        S.FUSED_FRAME = old


def _bounded(case, figure, value, bound):
    print(f"CHURN {case} {figure} {value / bound:.3f}")
    assert value < bound, (case, figure, value, bound)


def _lists_close(case, name, got, want, rtol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    worst = float((np.abs(got - want) / (rtol * np.abs(want))).max())
    print(f"CHURN {case} {name} {worst:.3f}")
    np.testing.assert_allclose(got, want, rtol=rtol)


@pytest.mark.parametrize("tag", ["churn", "target", "all"])
def test_fused_against_the_fixture(tag):
    s = _setup()
    z = s["z"]
    kw = dict(churn=dict(S_churn=8), target=dict(target=s["target"]), all=dict(guidance=0.7, S_churn=8, target=s["target"]))[tag]
    x, mse, mse_pred, cache = _sample(1, **kw)
    _bounded(f"fixture[{tag}]", "frame", rel(x, z[tag + "_x"]), 5e-2)
    assert cache["n_context_frames"] == int(z[tag + "_cache_n_ctx"])
    assert _kv_len(cache) == int(z[tag + "_cache_attn_frames"]) * 64          # 8x8 tokens per frame at the video-attention level
    if "target" in kw:
        assert len(mse) == len(mse_pred) == len(z[tag + "_mse"]) == 4
        _lists_close(f"fixture[{tag}]", "mse", mse, z[tag + "_mse"], 5e-2)
        _lists_close(f"fixture[{tag}]", "mse_pred", mse_pred, z[tag + "_mse_pred"], 5e-2)
    else:
        assert mse == [] and mse_pred == []


CHURN_CASES = {"S_churn=8": dict(S_churn=8),                       # gamma clamped at sqrt(2) - 1
               "S_churn=1": dict(S_churn=1),                       # gamma = 0.25
               "S_churn=8,S_max=50": dict(S_churn=8, S_max=50)}    # step 0 (sigma 80) not churned, the rest are


def _agree(case, a, b):
    _bounded(case, "frame", rel(a[0], b[0].cpu().numpy()), 1e-5)
    assert torch.isfinite(a[0]).all()
    assert len(a[1]) == len(b[1]) and len(a[2]) == len(b[2])
    if b[1]:
        _lists_close(case, "mse", a[1], b[1], 1e-4)
        _lists_close(case, "mse_pred", a[2], b[2], 1e-4)
    assert a[3]["n_context_frames"] == b[3]["n_context_frames"] and _kv_len(a[3]) == _kv_len(b[3])


@pytest.mark.parametrize("guidance", [1, 0.7])
@pytest.mark.parametrize("with_target", [False, True])
@pytest.mark.parametrize("churn", list(CHURN_CASES))
def test_fused_against_tensor_expressions(churn, with_target, guidance):
    s = _setup()
    kw = dict(CHURN_CASES[churn], guidance=guidance)
    if with_target:
        kw["target"] = s["target"]
    _agree(f"fused-vs-expressions[{churn},target={int(with_target)},g={guidance}]", _sample(1, **kw), _sample(0, **kw))


@pytest.mark.parametrize("with_target", [False, True])
def test_draw_order(with_target):
    """No noise given: the initial draw, then one randn_like per churned step in step order -- the generator state after the seed
    is consumed identically by both loops."""
    s = _setup()
    kw = dict(S_churn=8, S_max=50)
    if with_target:
        kw["target"] = s["target"]
    outs = []
    for fused in (1, 0):
        torch.manual_seed(7)
        outs.append(_sample(fused, given_noise=False, **kw))
    _agree(f"draw-order[target={int(with_target)}]", *outs)


def test_probe_reads_nothing_back_inside_the_loop(monkeypatch):
    s = _setup()
    calls = [0]
    item = torch.Tensor.item

    def counting(self):
        calls[0] += 1
        return item(self)
    monkeypatch.setattr(torch.Tensor, "item", counting)
    x, mse, mse_pred, _ = _sample(1, target=s["target"], S_churn=8)
    monkeypatch.undo()
    assert calls[0] == 0, f"{calls[0]} .item() calls in a probed frame"
    assert len(mse) == len(mse_pred) == KW["num_steps"]
    assert all(type(v) is float for v in mse + mse_pred)


def test_probe_leaves_the_cache_alone():
    s = _setup()
    a = _sample(1)[0]
    cache = _fork(s["cache0"])
    before = (cache["n_context_frames"], _kv_len(cache))
    _, mse, _, back = _sample(1, cache=cache, target=s["target"], S_churn=8, guidance=0.7)
    assert len(mse) == 4 and back is cache
    assert (cache["n_context_frames"], _kv_len(cache)) == before
    b = _sample(1, cache=cache)[0]
    _bounded("probe-leaves-cache", "frame", rel(b, a.cpu().numpy()), 1e-5)


def test_churned_frame_is_one_call_of_the_net():
    """The capture; every other evaluation is a replay and the cache update comes from the last replay's shadow cache."""
    s = _setup()
    net = s["net"]
    calls = [0]
    forward = net.forward

    def counting(*a, **k):
        calls[0] += 1
        return forward(*a, **k)
    net.forward = counting
    try:
        _, _, _, cache = _sample(1, S_churn=8)
    finally:
        del net.forward
    assert calls[0] == 1, f"{calls[0]} calls of the net's forward in a churned frame"
    assert cache["n_context_frames"] == s["cache0"]["n_context_frames"] + 1
