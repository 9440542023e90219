"""The VAE losses without a GPU: the restatement (tests/vae_losses_cpu_restatement.py) against fixture G21 (the reference's own
float64 run), the crafted key sets' properties, the torch fall-back of the public functions against the same fixture, and the host
side of the launch (loop order and merged dimensions)."""
import functools
import os

import numpy as np
import pytest
import torch

import vae_losses_cpu_restatement as R
import vae_losses_gen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSSES = ("gauss", "l1", "mse")


@functools.lru_cache(maxsize=None)
def g21():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g21_vae_losses.npz")))


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@functools.lru_cache(maxsize=None)
def fused64(case):
    """The float64 yardstick of one fused case, computed once: (losses, mean |term|, gradients of sum COTS[i] loss_i)."""
    return R.fused(*G.inputs(case), G.COTS)


def g21_fused_grad(z, case, which):
    """sum_i COTS[i] * the stored unit-cotangent gradient of loss i (None when the case stores norms only)."""
    if f"{case}/gauss/{which}" not in z:
        return None
    g = G.COTS[0] * z[f"{case}/gauss/{which}"].astype(np.float64)
    if which != "dlogvar":
        g = g + G.COTS[1] * z[f"{case}/l1/{which}"] + G.COTS[2] * z[f"{case}/mse/{which}"]
    return torch.from_numpy(g)


@pytest.mark.parametrize("case", list(G.CASES))
def test_fused_restatement_against_g21(case):
    z = g21()
    losses, termabs, grads = fused64(case)
    for name, v, ta in zip(LOSSES, losses, termabs):
        assert abs(v - float(z[f"{case}/{name}"])) <= 1e-12 * abs(v), name
        assert abs(ta - float(z[f"{case}/termabs/{name}"])) <= 1e-12 * ta
    for which, g in zip(("dmean", "dlogvar", "dtarget"), grads):
        want = g21_fused_grad(z, case, which)
        if want is not None:
            assert rel(g, want) <= 2e-7, which                 # the fixture stores float32
        else:                                                  # norms only: each loss alone
            for i, name in enumerate(LOSSES):
                if which == "dlogvar" and name != "gauss":
                    continue
                cots = tuple(1.0 if j == i else 0.0 for j in range(3))
                gi = R.fused(*G.inputs(case), cots)[2][("dmean", "dlogvar", "dtarget").index(which)]
                assert abs(gi.norm().item() - float(z[f"{case}/{name}/norm/{which}"])) <= 1e-12 * gi.norm().item(), (name, which)


@pytest.mark.parametrize("wk", list(G.WORSTK))
def test_selection_restatement_against_g21(wk):
    z = g21()
    case, percent = G.WORSTK[wk]
    mean, _, target = G.inputs(case)
    k = G.worst_k(mean.numel(), percent)
    sel = R.select(mean, target, k)
    assert k == int(z[f"{wk}/k"]) and int(sel["thr"]) == int(z[f"{wk}/thr"])
    assert sel["count_gt"] == int(z[f"{wk}/count_gt"]) and sel["count_eq"] == int(z[f"{wk}/count_eq"]) == 1
    loss = R.worst_k_loss(sel)
    assert abs(loss - float(z[f"{wk}/loss"])) <= 2e-7 * loss     # e rounded to float32 once: 2^-24 relative per term
    g = R.worst_k_grad(sel, 1.0)
    assert int((g != 0).sum()) == int(z[f"{wk}/nonzero"]) == k
    if f"{wk}/drecon" in z:
        want = z[f"{wk}/drecon"].astype(np.float64).ravel()
        assert np.array_equal(g != 0, want != 0)
        assert np.all(np.abs(g - want) <= 2e-7 * np.abs(want))
    else:
        assert abs(np.linalg.norm(g) - float(z[f"{wk}/norm/drecon"])) <= 2e-7 * np.linalg.norm(g)
    if wk == "mid_all":                                          # k = numel: the loss is mse_loss
        assert abs(loss - float(z["mid/mse"])) <= 2e-7 * loss
    if wk == "tiny_k1":                                          # k = 1: the loss is the maximum
        assert loss == float(sel["e"].max())


def test_crafted_key_sets_have_the_properties_they_are_named_for():
    sel = R.select(*G.crafted("low_digit"))
    assert len(set(sel["key"] >> 10)) == 1 and len(set(sel["key"])) == 500 and sel["count_eq"] == 1
    sel = R.select(*G.crafted("spread"))
    assert (sel["key"] == 0).sum() == 40 and ((sel["key"] > 0) & (sel["key"] < 0x00800000)).sum() >= 10     # zeros, denormals
    assert len(set(sel["key"] >> 23)) > 30 and np.isfinite(R.worst_k_loss(sel))
    sel = R.select(*G.crafted("spread_inf"))
    assert (sel["key"] == 0x7f800000).sum() == 2 and R.worst_k_loss(sel) == float("inf")
    sel = R.select(*G.crafted("ties"))
    assert sel["count_eq"] > sel["k"] - sel["count_gt"] > 0 and len(set(sel["key"])) < 64
    w = R.worst_k_weights(sel)
    assert abs(w.sum() - sel["k"]) <= 1e-9 * sel["k"]
    g = R.worst_k_grad(sel, G.WK_COT)
    d64 = sel["d"].astype(np.float64)
    assert abs(g.sum() - G.WK_COT * 2 / sel["k"] * (w * d64).sum()) <= 1e-12 * np.abs(g).sum()
    sel = R.select(*G.crafted("equal"))
    assert sel["thr"] == 0 and sel["count_gt"] == 0 and sel["count_eq"] == sel["key"].size
    assert R.worst_k_loss(sel) == 0.0 and not R.worst_k_grad(sel, G.WK_COT).any()
    sel = R.select(*G.crafted("nan"))
    assert np.isnan(R.worst_k_loss(sel)) and sel["thr"] < 0x7f800000 and (sel["key"] > 0x7f800000).sum() == 1


@pytest.mark.parametrize("case", list(G.CASES))
def test_cpu_fallback_of_the_public_functions(case):
    """CPU tensors take the torch formula of the reference: float64 operands reproduce the fixture, float32 operands stay inside
    the bounds the GPU tests use; a CPU call never raises for being a CPU call."""
    from autoregressive_diffusion_amd import vae_losses as V
    z = g21()
    for dtype, ltol, gtol in ((torch.float64, 1e-12, 2e-7), (torch.float32, 1e-5, 2e-6)):
        m, lv, tg = (t.to(dtype).requires_grad_(True) for t in G.inputs(case))
        trio = V.recon_losses(m, lv, tg)
        singles = (V.GaussianLoss(m, lv, tg), V.l1_loss(m, tg), V.mse_loss(m, tg))
        for name, a, b in zip(LOSSES, trio, singles):
            assert a.dim() == 0 and a.dtype == dtype and torch.equal(a, b)
            assert abs(a.item() - float(z[f"{case}/{name}"])) <= ltol * float(z[f"{case}/termabs/{name}"]), (name, dtype)
        sum(c * v for c, v in zip(G.COTS, trio)).backward()
        _, _, want = fused64(case)
        for g, w in zip((m.grad, lv.grad, tg.grad), want):
            assert rel(g, w) <= gtol
    for wk, (c, percent) in G.WORSTK.items():
        if c != case:
            continue
        m, _, tg = G.inputs(case)
        m.requires_grad_(True)
        loss = V.worst_k_percent_loss(m, tg, percent=percent)
        loss.backward()
        assert abs(loss.item() - float(z[f"{wk}/loss"])) <= 1e-5 * float(z[f"{wk}/loss"])
        assert int((m.grad != 0).sum()) == int(z[f"{wk}/k"])
    assert V.worst_k(9690, 0.5) == 48 and V.worst_k(9690, 0.2) == 19 and V.worst_k(105, 0.5) == 1 and V.worst_k(49104, 100.0) == 49104


def test_launch_layout_on_the_host():
    """_layout: flat when every operand is contiguous and 16-byte aligned; otherwise the loop runs in the memory order of the first
    operand that is not contiguous, and dimensions every operand steps through with one stride are merged."""
    from autoregressive_diffusion_amd import vae_losses as V
    a, b = torch.zeros(2, 3, 4, 6, 8), torch.zeros(2, 3, 4, 6, 8)
    nd, size, stride = V._layout([a, None, b])
    assert (nd, list(size), stride) == (1, [1152], None)
    cl = torch.zeros(2, 4, 6, 8, 3).permute(0, 4, 1, 2, 3)                      # the scripts' frames: 'b t h w c -> b c t h w'
    nd, size, stride = V._layout([a, b, cl])
    assert nd == 3 and list(size) == [2, 4 * 6 * 8, 3]                          # (b, t h w, c), c innermost as in memory
    assert list(stride) == [576, 1, 192] * 2 + [576, 3, 1]
    nd, size, stride = V._layout([a, None, cl, a, None, cl])
    assert nd == 3 and list(stride)[3:6] == [0, 0, 0] and list(stride)[12:15] == [0, 0, 0] and list(stride)[15:] == [576, 3, 1]
    off = torch.zeros(1153)[1:].view(2, 3, 4, 6, 8)                              # contiguous but 4 bytes off a 16-byte boundary
    nd, size, stride = V._layout([off, a])
    assert nd == 1 and list(size) == [1152] and list(stride) == [1, 1]
    ex = torch.zeros(1, 3, 1, 1, 8).expand(2, 3, 4, 6, 8)                        # broadcast operands keep their zero strides
    nd, size, stride = V._layout([ex, a])
    assert nd == 4 and list(size) == [3, 8, 2, 24] and list(stride) == [8, 1, 0, 0, 192, 1, 576, 8]      # (c, w, b, t h)
    flat = {}
    for idx in np.ndindex(*[int(s) for s in size]):                              # every logical element exactly once in `a`
        o = sum(i * st for i, st in zip(idx, list(stride)[nd:]))
        flat[o] = flat.get(o, 0) + 1
    assert sorted(flat) == list(range(1152)) and set(flat.values()) == {1}
