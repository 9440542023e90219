"""The LPIPS module (autoregressive_diffusion_amd/lpips.py) without a GPU: the state-dict layout, the frozen parameters, the refusals,
and its torch formula against the float64 restatement (tests/lpips_cpu_restatement.py)."""
import pytest
import torch

import lpips_cpu_restatement as R


def L():
    from autoregressive_diffusion_amd import lpips
    return lpips


def loaded(dtype=torch.float32):
    return L().LPIPS(net="alex", weights=R.seeded_weights(3)).to(dtype)


def test_state_dict_keys_are_the_table():
    m = L().LPIPS()
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == R.key_table() == L().KEYS
    assert torch.equal(sd["scaling_layer.shift"].flatten(), torch.tensor(R.SHIFT))
    assert torch.equal(sd["scaling_layer.scale"].flatten(), torch.tensor(R.SCALE))
    for i in range(5):          # the heads are registered twice: one tensor under two names
        assert sd[f"lin{i}.model.1.weight"].data_ptr() == sd[f"lins.{i}.model.1.weight"].data_ptr()


@pytest.mark.parametrize("which", ["both", "lin", "lins"])
def test_aliases_load(which, tmp_path):
    sd = R.seeded_weights(5)
    if which == "lin":
        sd = {k: v for k, v in sd.items() if not k.startswith("lins.")}
    if which == "lins":
        sd = {k: v for k, v in sd.items() if not (k.startswith("lin") and not k.startswith("lins."))}
    m = L().LPIPS()
    m.load_state_dict(sd, strict=True)
    full = R.seeded_weights(5)
    for k, v in m.state_dict().items():
        assert torch.equal(v, full[k]), k
    path = tmp_path / "w.pt"
    torch.save(sd, path)
    m2 = L().LPIPS(net="alex", weights=str(path))
    for k, v in m2.state_dict().items():
        assert torch.equal(v, full[k]), k


def test_parameters_are_frozen_and_eval_stays():
    m = loaded()
    assert list(m.parameters()) and not any(p.requires_grad for p in m.parameters())
    assert not m.training and not m.train().training and not any(c.training for c in m.modules())
    a, b = R.images((1, 31, 31), 0)
    m(a.requires_grad_(True), b).sum().backward()
    assert all(p.grad is None for p in m.parameters()) and a.grad is not None


def test_refusals():
    lp = L()
    for net in ("vgg", "squeeze"):
        with pytest.raises(NotImplementedError):
            lp.LPIPS(net=net)
    a, b = R.images((2, 31, 31), 0)
    with pytest.raises(RuntimeError):
        lp.LPIPS()(a, b)
    m = loaded()
    assert tuple(m(a, b).shape) == (2, 1, 1, 1)
    with pytest.raises(ValueError):
        m(a[:, :, :30], b[:, :, :30])
    with pytest.raises(ValueError):
        m(a[:, :, :, :30], b[:, :, :, :30])
    with pytest.raises(ValueError):
        m(a, b[:1])
    with pytest.raises(ValueError):
        m(a, torch.cat([b, b], 3))


@pytest.mark.parametrize("shape", [(2, 31, 64), (1, 67, 45)], ids=lambda s: "x".join(map(str, s)))
def test_forward_torch_in_float64_is_the_restatement(shape):
    sd = R.seeded_weights(3)
    m = loaded(torch.float64)
    a, b = R.images(shape, 1)
    c = R.cot(shape[0])
    want = R.run(sd, a, b, torch.float64, c)
    x, y = a.double().requires_grad_(True), b.double().requires_grad_(True)
    out = m.forward_torch(x, y)
    assert out.dtype == torch.float64 and tuple(out.shape) == (shape[0], 1, 1, 1)
    (out * c.double()).sum().backward()
    for k, got in (("value", out.detach()), ("d_in0", x.grad), ("d_in1", y.grad)):
        e = ((got - want[k]).norm() / want[k].norm()).item()
        print(f"{shape} {k}: rel L2 {e:.2e}")
        assert e <= 1e-12, (k, e)          # float64 against float64: a few thousand roundings of 1.1e-16
    assert bool(torch.equal(m(a.double(), b.double()), out.detach()))          # CPU tensors take forward_torch


def test_normalize_is_the_call_on_2x_minus_1():
    m = loaded(torch.float64)
    a, b = R.images((2, 31, 33), 2)
    a, b = (a.double() + 1) / 2, (b.double() + 1) / 2
    assert torch.equal(m(a, b, normalize=True), m(2 * a - 1, 2 * b - 1))
    want = R.distance(R.seeded_weights(3), a, b, torch.float64, normalize=True)
    assert ((m(a, b, normalize=True) - want).norm() / want.norm()).item() <= 1e-12


def test_an_all_zero_pixel_takes_no_gradient():
    """torch's own adjoint of the norm is NaN there; the module's formula (and the kernels) give that pixel a zero gradient."""
    fa = torch.randn(1, 64, 3, 3, dtype=torch.float64)
    fa[:, :, 1, 1] = 0
    fa.requires_grad_(True)
    fb = torch.randn(1, 64, 3, 3, dtype=torch.float64)
    R.head(fa, fb, torch.rand(1, 64, 1, 1, dtype=torch.float64)).sum().backward()
    assert bool(torch.isfinite(fa.grad).all()) and not bool(fa.grad[:, :, 1, 1].any()) and bool(fa.grad[:, :, 0, 0].any())


def test_packed_weights_are_cached_until_a_parameter_changes():
    m = loaded()
    pk = m._pack(torch.device("cpu"))
    assert m._pack(torch.device("cpu")) is pk
    w = m.net.slice2._modules["3"].weight
    assert torch.equal(pk["fwd"][1], w.permute(2, 3, 1, 0).reshape(25, 64, 192))
    assert torch.equal(pk["bwd"][1], w.flip(2, 3).permute(2, 3, 0, 1).reshape(25, 192, 64))
    with torch.no_grad():
        w.mul_(2)
    pk2 = m._pack(torch.device("cpu"))
    assert pk2 is not pk and torch.equal(pk2["fwd"][1], 2 * pk["fwd"][1])
    m.load_state_dict(R.seeded_weights(4))
    assert torch.equal(m._pack(torch.device("cpu"))["lin"][0], R.seeded_weights(4)["lin0.model.1.weight"].flatten())
