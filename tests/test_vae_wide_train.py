"""CPU checks of wide VAE training: the float64 training restatement (tests/vae_train_cpu_restatement.py) against fixture G24 (the
reference in float64 at a 72-channel block), the `VAE.wide_training()` switch, every data-gradient pack layout of
autoregressive_diffusion_amd/vae_train.py applied through a restatement of the kernel's indexing against autograd in float64,
and the declaration and binding of the new C entry points.  No kernel runs."""
import copy
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import vae_wide_oracle as O  # noqa: E402
import vae_wide_encoder_oracle as E  # noqa: E402
import vae_wide_train_oracle as WT  # noqa: E402
import vae_train_cpu_restatement as R  # noqa: E402

F64 = torch.float64
NEW = ("oniris_vae_wide_act_bwd", "oniris_vae_wide_conv_b_bwd", "oniris_vae_wide_conv3_wgrad_bwd", "oniris_vae_wide_down_bwd",
       "oniris_vae_wide_up_bwd", "oniris_vae_wide_lin_wgrad_bwd")


def g24():
    z = np.load(os.path.join(HERE, "golden", "g24_vae_wide_train.npz"))
    kw = dict(channels=z["kw_channels"].tolist(), n_res_blocks=int(z["kw_n_res_blocks"]),
              time_compressions=z["kw_time_compressions"].tolist(), spatial_compressions=z["kw_spatial_compressions"].tolist())
    return z, kw


def g24_vae():
    from autoregressive_diffusion_amd.vae import VAE
    z, kw = g24()
    return z, kw, O.seed_params(VAE(**kw), int(z["seed"]))


def g24_stride(numel):
    s = -(-numel // 4096)
    return s + 1 - (s & 1)


def g24_grad_error(z, name, grad):
    """The distance of a float64 gradient from G24's: rel L2 over what the fixture stores of it (all of a gradient of up to 8192
    elements; else every stride-th element, with the relative errors of the L2 norm and the sum over all of it)."""
    want, g = torch.from_numpy(z["grad/" + name]), grad.detach().double().cpu().reshape(-1)
    if "norm/" + name not in z.files:
        return O.rel_l2(g, want.reshape(-1))
    norm, total = float(z["norm/" + name]), float(z["sum/" + name])
    return max(O.rel_l2(g[::g24_stride(g.numel())], want), abs(g.norm().item() - norm) / norm, abs(g.sum().item() - total) / norm)


def test_restatement_matches_g24():
    """Both are float64, so only the order of operations differs: 1e-10 on the outputs and on every parameter gradient."""
    z, kw, vae = g24_vae()
    assert np.allclose(O.param_sums(vae), z["param_sums"], rtol=1e-9, atol=1e-9)
    assert vae.encoder.out_channels == [8, 72, 8] and vae.encoder.group_sizes == [2, 2, 1] and vae.decoder.group_sizes == [1, 2, 2]
    x = (torch.from_numpy(z["frames"]).double() / 127.5 - 1).permute(0, 4, 1, 2, 3)
    outs, grads = R.grads(vae.state_dict(), kw, x, torch.from_numpy(z["t_sample"]), torch.from_numpy(z["noise"]))
    for k in ("mean", "r_mean", "r_logvar"):
        assert z[k].dtype == np.float64 and O.rel_l2(outs[k], z[k]) <= 1e-10, k
    names = [n for n, _ in vae.named_parameters()]
    assert sorted(grads) == sorted(names) and len([k for k in z.files if k.startswith("norm/")]) == 6
    for n in names:
        assert g24_grad_error(z, n, grads[n]) <= 1e-10, n


def test_switch():
    from autoregressive_diffusion_amd.vae import VAE
    wide = VAE(channels=[3, 16, 64, 256, 8], n_res_blocks=1, time_compressions=[1, 2, 2, 1], spatial_compressions=[1, 2, 2, 2]).train()
    assert wide._wide_training is False
    keys, kwargs = set(wide.state_dict()), dict(wide.kwargs)
    x = torch.zeros(1, 3, 8, 16, 16)
    with pytest.raises(NotImplementedError, match=r"256 channels.*decoder.*edm2\.vae"):    # the CPU model's refusal, switch off
        wide(x)
    assert wide.wide_training() is wide and wide._wide_training is True
    assert set(wide.state_dict()) == keys and wide.kwargs == kwargs and "wide_training" not in str(kwargs)
    assert copy.deepcopy(wide)._wide_training is True
    with pytest.raises(NotImplementedError, match=r"256 channels.*HIP kernels only.*edm2\.vae"):    # still the device refusal
        wide(x)
    assert wide.wide_training(False)._wide_training is False and copy.deepcopy(wide)._wide_training is False
    g23ish = VAE(channels=[3, 72, 160, 8], n_res_blocks=1).train()
    with pytest.raises(NotImplementedError, match=r"160 channels.*edm2\.vae"):
        g23ish(torch.zeros(1, 3, 4, 8, 8))


def test_switch_off_message_on_the_training_path(monkeypatch):
    """The refusal of the training path itself (behind the device check, which a CPU model never passes): same type, the old text,
    one sentence naming the switch behind it."""
    from autoregressive_diffusion_amd.vae import VAE
    wide = VAE(channels=[3, 72, 160, 8], n_res_blocks=1).train()
    monkeypatch.setattr(VAE, "_encoder_device", lambda self, what, x=None: torch.device("cpu"))
    with pytest.raises(NotImplementedError) as e:
        wide(torch.zeros(1, 3, 4, 8, 8))
    msg = str(e.value)
    assert re.search(r"160 channels.*edm2\.vae", msg) and re.search(r"160 channels.*decoder.*edm2\.vae", msg)
    assert "inference only (eval mode or torch.no_grad())" in msg and msg.rstrip().endswith("for this model")
    assert "wide_training()" in msg.split("edm2.vae")[-1]


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


@pytest.mark.parametrize("g", [1, 2, 4])
@pytest.mark.parametrize("C", [72, 128])
def test_conv_dgrad_packs(C, g):
    """Conv A's data gradient is the forward kernel on D = [da ++ g zero frames] with the repacked weights: at T = 2g the first
    group also feeds the detached prefix (dropped) and the last group has a single reader.  Conv B's is a 3x3 conv on flipped,
    transposed weights.  Against autograd in float64; the weights are fp32 values, so the packs hold them exactly."""
    from autoregressive_diffusion_amd import vae_train
    gen = torch.Generator().manual_seed(100 * C + g)
    B, T, H, W = 1, 2 * g, 3, 4
    wa, wb = _randn(gen, C * g, C, 2 * g, 3, 3) / (18 * g * C) ** 0.5, _randn(gen, C, C, 1, 3, 3) / (9 * C) ** 0.5
    wda, wdb, zb = vae_train._pack_dgrad_wide(wa, wb, C, g)
    CP, CinP = -(-C // 32) * 32, C + (C & 1)
    assert tuple(wda.shape) == (2 * g, 3, 3, CinP, g, CP) and tuple(wdb.shape) == (3, 3, CinP, CP) and tuple(zb.shape) == (g, CP)
    assert wda[:, :, :, C:].abs().sum() == 0 and wda[..., C:].abs().sum() == 0 and zb.abs().sum() == 0
    assert wdb[:, :, C:].abs().sum() == 0 and wdb[..., C:].abs().sum() == 0
    y = _randn(gen, B, T, H, W, C).double().requires_grad_(True)
    da = _randn(gen, B, T, H, W, C).double()
    S = torch.cat((y[:, :g].detach(), y), dim=1)
    (O.conv_a(S, wa, torch.zeros(C * g), g) * da).sum().backward()
    D = torch.cat((da, torch.zeros(B, g, H, W, C, dtype=F64)), dim=1)
    assert O.rel_l2(WT.conv_a_packed(D, wda, zb, g, C), y.grad) <= 1e-12
    u = _randn(gen, B, T, H, W, C).double().requires_grad_(True)
    (O.conv_b(u, torch.zeros_like(u), wb, torch.zeros(C)) * da).sum().backward()
    assert O.rel_l2(WT.conv3_packed(da, wdb, C), u.grad) <= 1e-12


@pytest.mark.parametrize("tc,sc", [(1, 1), (2, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("Cin,Cout", [(72, 128), (128, 72), (72, 8), (8, 72)])
def test_lin_dgrad_packs(Cin, Cout, tc, sc):
    """The adjoint of `down` (and of `out` at tc = sc = 1) as an `up` on (W + the area matrix)^T, and the adjoint of `up` as a `down`
    without residual on W^T, against autograd in float64.  The area matrix holds 1 / len in fp32, so 1e-7."""
    from autoregressive_diffusion_amd import vae_train
    gen = torch.Generator().manual_seed(1000 * Cin + 10 * Cout + 2 * tc + sc)
    B, T, H, W = 1, 2, 3, 2
    npos = tc * sc * sc
    K = Cin * npos
    wd = _randn(gen, Cout, K, 1, 1, 1) / K ** 0.5
    x = _randn(gen, B, T * tc, H * sc, W * sc, Cin)
    dy = _randn(gen, B, T, H, W, Cout)
    _, dx, _, _ = WT.lin_grads(E.down, x, wd, torch.zeros(Cout), (dy,), tc=tc, sc=sc)
    w, zb = vae_train._pack_down_dgrad(wd, Cin, Cout, tc, sc)
    assert tuple(w.shape) == (Cout + (Cout & 1), npos, -(-Cin // 32) * 32) and zb.abs().sum() == 0
    assert O.rel_l2(WT.up_packed(dy, w, zb, Cout, Cin, tc, sc), dx) <= 1e-7


@pytest.mark.parametrize("C", [72, 128])
def test_up_dgrad_pack(C):
    from autoregressive_diffusion_amd import vae_train
    gen = torch.Generator().manual_seed(C)
    for tc, sc in ((1, 1), (2, 1), (1, 2), (2, 2)):
        npos = tc * sc * sc
        wu = _randn(gen, C * npos, C, 1, 1, 1) / C ** 0.5
        x, dup = _randn(gen, 1, 2, 3, 2, C), _randn(gen, 1, 2 * tc, 3 * sc, 2 * sc, C)
        _, dx, _, _ = WT.lin_grads(O.up, x, wu, torch.zeros(C * npos), (dup,), tc=tc, sc=sc)
        w, zb = vae_train._pack_up_dgrad(wu, C, tc, sc)
        assert tuple(w.shape) == (npos, C + (C & 1), -(-C // 32) * 32) and zb.abs().sum() == 0
        assert O.rel_l2(WT.down_packed(dup, w, zb, C, C, tc, sc), dx) <= 1e-12


def test_entry_points_are_bound_and_declared():
    """Every new symbol is exported, bound, and declared in include/oniris.h with as many arguments as _lib gives it."""
    from autoregressive_diffusion_amd import _lib
    header = open(os.path.join(os.path.dirname(HERE), "include", "oniris.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTED and callable(getattr(_lib.lib, name))
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib._SIGS[name][1]) == len(getattr(_lib.lib, name).argtypes), name
    assert _lib.lib.oniris_abi_version() == 14
