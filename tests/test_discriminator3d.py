"""CPU checks of the 3-D discriminator (autoregressive_diffusion_amd/discriminator.py Discriminator3D): the float64 restatement
(tests/disc_cpu_restatement.py:disc3d) against the reference's fixture G20 (rel L2 <= 1e-6: the fixture holds float32 roundings of
float64 results, 1e-6 is about 10 ulp of that), the state-dict surface, the domain errors that can be raised without a GPU, and the
per-stage expectations of tests/disc3d_cpu_restatement.py against torch autograd in float64.  The kernels are
tests/test_discriminator3d_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

import disc_paramgen as G
import disc3d_paramgen as G3
import disc_cpu_restatement as R
import disc3d_cpu_restatement as R3

TOL = 1e-6
F64 = torch.float64


@pytest.mark.parametrize("name", list(G3.G20_NETS))
def test_restatement_equals_g20(name):
    cin, widths, shape, seed = G3.G20_NETS[name]
    fx = R.fixture("g20_disc3d.npz", name)
    out = R3.run3d(G.fill(G.disc3d_shapes(cin, widths), seed), G.inputs(shape, seed), len(widths), F64)
    assert tuple(out["logits"].shape) == G3.G20_LOGITS[name]
    zero = ["grad/" + k for k in G3.G20_ZERO_BIAS[name]]
    assert zero == [k for k in out if k.startswith("grad/") and k.endswith("conv1.bias")
                    and out[k].numel() == 32], "conv1 with 32 output channels: one channel per group"
    compared = 0
    for k, v in fx.items():
        if k.startswith("ref32_rel/") or k in ("keys", "shapes"):
            continue
        assert k in out, k
        if k in zero:
            wk = k.replace("conv1.bias", "conv1.weight")
            scale = out[wk].norm() if wk in out else out[wk.replace("grad/", "gradnorm/")]
            assert out[k].abs().max() <= 1e-9 * scale and v.abs().max() <= 1e-9 * scale, k
        else:
            assert tuple(out[k].shape) == tuple(v.shape), k
            assert R.rel(out[k], v) <= TOL, (k, R.rel(out[k], v))
            assert ("ref32_rel/" + k) in fx
        compared += 1
    assert compared == len(out) and not any("conv_norm_out" in k for k in out)
    big = [k for k in out if k.startswith("gradnorm/")]
    assert all(k.replace("gradnorm/", "gradtaps/") in out and k.replace("gradnorm/", "gradhead/") in out for k in big)


def test_state_dict_surface():
    from autoregressive_diffusion_amd.discriminator import Discriminator3D
    for name, (cin, widths, _, seed) in G3.G20_NETS.items():
        fx = R.fixture("g20_disc3d.npz", name)
        want = dict(zip(fx["keys"].tolist(), fx["shapes"].tolist()))
        net = Discriminator3D(cin, widths)
        assert {k: ",".join(map(str, v.shape)) for k, v in net.state_dict().items()} == want
        net.load_state_dict(G.fill(G.disc3d_shapes(cin, widths), seed), strict=True)
        assert any(k.endswith("filt") for k in want) == (len(widths) > 1)


def test_torch_path_on_cpu_equals_g20():
    """With CPU tensors Discriminator3D stays the torch code, in the tensors' dtype: net a3 in float64 against G20."""
    from autoregressive_diffusion_amd.discriminator import Discriminator3D
    cin, widths, shape, seed = G3.G20_NETS["a3"]
    net = Discriminator3D(cin, widths)
    net.load_state_dict(G.fill(G.disc3d_shapes(cin, widths), seed), strict=True)
    with torch.no_grad():
        y = net.double()(G.inputs(shape, seed).double())
    assert y.dtype == F64 and R.rel(y, R.fixture("g20_disc3d.npz", "a3")["logits"]) <= TOL


def test_domain():
    """Constructing is legal for whatever the torch path takes; the native domain is checked where it can be without a GPU."""
    from autoregressive_diffusion_amd import discriminator as d
    for cin, widths in ((9, (32,)), (3, (288, 288)), (3, (64, 96))):          # (widths are multiples of 32: nn.GroupNorm(32, .))
        net = d.Discriminator3D(cin, widths)
        assert net.widths == list(widths)
    d.Discriminator3D(3, (64, 96))._native_domain()
    d.Discriminator3D(8, (32, 256, 96))._native_domain()
    with pytest.raises(NotImplementedError, match="1..8"):
        d.Discriminator3D(9, (32,))._native_domain()
    with pytest.raises(NotImplementedError, match="multiples of 32"):
        d.Discriminator3D(3, (64, 320))._native_domain()
    with pytest.raises(NotImplementedError, match="multiples of 32"):
        d.Discriminator3D(3, (288, 288))._native_domain()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        d._gn_check(torch.zeros(1, 1, 1, 1, 32))
    d._gn_check(torch.zeros(1, 1, 1, 1, 64))
    d._gn_check(torch.zeros(2, 1, 1, 1, 32))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):          # torch's own, on the CPU path
        d.Discriminator3D(3, (32,))(torch.zeros(1, 3, 1, 1, 1))
    assert d._nslab3(10 ** 6, 27 * 256 * 256 + 256) * 4 * (27 * 256 * 256 + 256) <= d._SLAB_BYTES
    assert d._nslab3(5, 100) == 5 and d._nslab3(10 ** 6, 100) == d._MAX_SLABS


# ---- the per-stage expectations against torch autograd in float64

def _g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("stride,shape", [(1, (2, 3, 5, 4, 3, 5)), (2, (2, 3, 5, 7, 4, 6)), (2, (1, 2, 1, 4, 4, 3))])
def test_conv_expectations(stride, shape):
    N, Cin, Cout, T, H, W = shape
    g = _g(1)
    x = torch.randn(N, Cin, T, H, W, generator=g, dtype=F64).requires_grad_(True)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g, dtype=F64).requires_grad_(True)
    b = torch.randn(Cout, generator=g, dtype=F64).requires_grad_(True)
    y = F.conv3d(x, w, b, stride=stride, padding=1)
    half = lambda n: (n - 1) // stride + 1
    assert tuple(y.shape[2:]) == (half(T), half(H), half(W))
    res = torch.randn(y.shape, generator=g, dtype=F64)
    v, m = R3.conv_terms(x.detach(), w.detach(), b.detach(), res, 0.7, stride)
    assert R.rel(v, (y.detach() + res) * 0.7) <= 1e-12 and bool((m >= v.abs() - 1e-12).all())
    ones = R3.conv_terms(torch.ones_like(x), torch.ones_like(w), stride=stride)[1]
    assert ones.max() <= 27 * Cin and ones.min() >= Cin                                  # the sum of |terms| counts the live taps
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    y.backward(dy)
    dx, mag, pairs = R3.dgrad_terms(dy, w.detach(), (T, H, W), stride)
    assert R.rel(dx, x.grad) <= 1e-12 and bool((mag >= dx.abs() - 1e-12).all())
    assert tuple(pairs.shape[2:]) == (T, H, W) and pairs.max() <= 27 and pairs.min() >= 0
    dw, db = R3.wgrad(x.detach(), dy, stride)
    assert R.rel(dw, w.grad) <= 1e-12 and R.rel(db, b.grad) <= 1e-12


def test_groupnorm_expectations():
    N, C, T, H, W = 2, 96, 2, 3, 5
    g = _g(2)
    z = (0.5 + 1.5 * torch.randn(N, C, T, H, W, generator=g, dtype=F64)).requires_grad_(True)
    gamma = (1 + 0.3 * torch.randn(C, generator=g, dtype=F64)).requires_grad_(True)
    beta = (0.3 * torch.randn(C, generator=g, dtype=F64)).requires_grad_(True)
    a = F.leaky_relu(F.group_norm(z, 32, gamma, beta, 1e-5), 0.2)
    mean, var, s, t, rstd = R3.gn_vectors(z.detach(), gamma.detach(), beta.detach())
    assert tuple(mean.shape) == (N, C) and bool((mean[:, 0] == mean[:, 2]).all()) and not bool((mean[:, 2] == mean[:, 3]).any())
    assert R.rel(R3.act(z.detach(), s, t), a) <= 1e-12
    da = torch.randn(a.shape, generator=g, dtype=F64)
    a.backward(da)
    dx, dgamma, dbeta, mag = R3.gn_backward(da, z.detach(), gamma.detach(), beta.detach(), mean, rstd)
    assert R.rel(dx, z.grad) <= 1e-12 and R.rel(dgamma, gamma.grad) <= 1e-12 and R.rel(dbeta, beta.grad) <= 1e-12
    assert bool((mag >= dx.abs() - 1e-12).all())


@pytest.mark.parametrize("shape", [(1, 7, 5), (4, 6, 8), (2, 2, 2), (1, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_blur_expectations(shape):
    from autoregressive_diffusion_amd.discriminator import BlurPooling3D
    g = _g(3)
    C = 4
    x = torch.randn(2, C, *shape, generator=g, dtype=F64).requires_grad_(True)
    y = BlurPooling3D(C).double()(x)
    v, m = R3.blur(x.detach(), terms=True)
    assert tuple(v.shape[2:]) == tuple((n - 1) // 2 + 1 for n in shape)
    assert R.rel(v, y) <= 1e-12 and bool((m >= v.abs() - 1e-12).all())
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    y.backward(dy)
    dx, mag = R3.blur_t(dy, shape, terms=True)
    assert R.rel(dx, x.grad) <= 1e-12 and bool((mag >= dx.abs() - 1e-12).all())
