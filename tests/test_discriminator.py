"""CPU checks of the discriminator (autoregressive_diffusion_amd/discriminator.py): the float64 restatement against the reference's
fixtures G18 / G19 (rel L2 <= 1e-6: the fixtures are float32 roundings of float64 results, 1e-6 is about 10 ulp of that), the
state-dict surface, the torch 3-D half, and the domain errors.  The kernels are tests/test_discriminator_gpu.py."""
import copy

import pytest
import torch

import disc_paramgen as G
import disc_cpu_restatement as R

TOL = 1e-6


def _zero_bias_keys(keys):
    return [k for k in keys if k.endswith("conv1.bias") and "discriminator3d" not in k]


@pytest.mark.parametrize("name", list(G.G18_NETS))
def test_restatement_equals_g18(name):
    cin, widths, shape, seed = G.G18_NETS[name]
    fx = R.fixture("g18_disc2d.npz", name)
    fx.update(R.fixture("g18_disc2d_grads.npz", name))
    out = R.run2d(G.fill(G.disc2d_shapes(cin, widths), seed), G.inputs(shape, seed), len(widths), torch.float64)
    compared = 0
    for k, v in fx.items():
        if k.startswith("ref32_rel/") or k in ("keys", "shapes"):
            continue
        assert k in out, k
        if k.endswith("num_batches_tracked"):
            assert int(out[k]) == int(v) == (3 if 'conv_norm_out' in k else 5)
        elif k.endswith("conv1.bias") and k.startswith("grad/"):
            scale = out[k.replace("conv1.bias", "conv1.weight")].norm()
            assert out[k].abs().max() <= 1e-9 * scale and v.abs().max() <= 1e-9 * scale, k
        else:
            assert tuple(out[k].shape) == tuple(v.shape), k
            assert R.rel(out[k], v) <= TOL, (k, R.rel(out[k], v))
        compared += 1
    assert compared == len(out) and not any(k.startswith("grad/conv_norm_out") for k in out)


def _mixed_run(name, dtype=torch.float64):
    cin, shape, seed = G.G19_NETS[name]
    p = {k: (v.to(dtype).requires_grad_(k.rsplit(".", 1)[1] in ("weight", "bias")) if v.is_floating_point() else v)
         for k, v in G.fill(G.mixed_shapes(cin), seed).items()}
    x = G.inputs(shape, seed).to(dtype).requires_grad_(True)
    logits, _ = R.mixed(p, x)
    (logits * G.cot(logits.shape, 0.3, dtype)).sum().backward()
    return p, x, logits.detach()


@pytest.mark.parametrize("name", list(G.G19_NETS))
def test_restatement_equals_g19(name):
    fx = R.fixture("g19_disc_mixed.npz", name)
    p, x, logits = _mixed_run(name)
    assert tuple(logits.shape) == (2, 2, 5, 8, 8)
    assert R.rel(logits, fx["logits"]) <= TOL and R.rel(x.grad, fx["dx"]) <= TOL
    norms = [k for k in fx if k.startswith("gradnorm/")]
    assert len(norms) == sum(1 for k, v in p.items() if v.requires_grad and "conv_norm_out" not in k)
    for k in norms:
        g = p[k[len("gradnorm/"):]].grad
        if k in ["gradnorm/" + z for z in _zero_bias_keys(p)]:
            assert g.norm() <= 1e-9 * p[k[len("gradnorm/"):].replace(".bias", ".weight")].grad.norm(), k
        else:
            assert abs(g.norm().item() - float(fx[k])) <= TOL * float(fx[k]), k
    for k in G.G19_FULL:
        assert R.rel(p[k].grad, fx["grad/" + k]) <= TOL, k
    pd = {k: v.detach() for k, v in p.items()}
    frames, recon = fx["frames"].double(), fx["recon"].double()
    for loss, flip in (("vae_loss", True), ("discriminator_loss", False)):
        got = R.mixed_loss(pd, frames, recon, flip).item()
        assert abs(got - float(fx[loss])) <= TOL * abs(float(fx[loss])), (loss, got, float(fx[loss]))


def test_state_dict_surface():
    from autoregressive_diffusion_amd.discriminator import Discriminator2D, MixedDiscriminator
    for name, (cin, widths, _, seed) in G.G18_NETS.items():
        fx = R.fixture("g18_disc2d.npz", name)
        want = dict(zip(fx["keys"].tolist(), fx["shapes"].tolist()))
        net = Discriminator2D(cin, widths)
        assert {k: ",".join(map(str, v.shape)) for k, v in net.state_dict().items()} == want
        net.load_state_dict(G.fill(G.disc2d_shapes(cin, widths), seed), strict=True)
    for name, (cin, _, seed) in G.G19_NETS.items():
        fx = R.fixture("g19_disc_mixed.npz", name)
        want = dict(zip(fx["keys"].tolist(), fx["shapes"].tolist()))
        net = MixedDiscriminator(cin)
        assert {k: ",".join(map(str, v.shape)) for k, v in net.state_dict().items()} == want
        params = G.fill(G.mixed_shapes(cin), seed)
        net.load_state_dict(params, strict=True)
        cp = copy.deepcopy(net)
        assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), cp.state_dict().values()))
        opt = torch.optim.AdamW(cp.parameters(), lr=1e-3)
        for q in cp.parameters():
            q.grad = torch.ones_like(q)
        torch.nn.utils.clip_grad_norm_(cp.parameters(), 1.0)
        opt.step()
        assert not torch.equal(cp.discriminator2d.conv_in.weight, net.discriminator2d.conv_in.weight)


@pytest.mark.parametrize("name", list(G.G19_NETS))
def test_torch_3d_half_on_cpu(name):
    from autoregressive_diffusion_amd.discriminator import MixedDiscriminator
    cin, shape, seed = G.G19_NETS[name]
    fx = R.fixture("g19_disc_mixed.npz", name)
    net = MixedDiscriminator(cin).train()
    net.load_state_dict(G.fill(G.mixed_shapes(cin), seed), strict=True)
    with torch.no_grad():
        y3 = net.double().discriminator3d(G.inputs(shape, seed).double())
    assert tuple(y3.shape) == (2, 2, 1, 8, 8)
    assert R.rel(y3, fx["logits"][:, :, 4:]) <= TOL and R.rel(y3, fx["d3_logits"]) <= TOL


def test_domain_errors():
    from autoregressive_diffusion_amd.discriminator import Discriminator2D, MixedDiscriminator
    with pytest.raises(NotImplementedError, match="edm2.vae"):
        Discriminator2D(3, (32,))(torch.zeros(1, 3, 8, 8))
    with pytest.raises(NotImplementedError, match="edm2.vae"):
        MixedDiscriminator(6)(torch.zeros(1, 6, 4, 16, 16))
    with pytest.raises(NotImplementedError, match="multiples of 32"):
        Discriminator2D(3, (48,))
    with pytest.raises(NotImplementedError, match="last two"):
        Discriminator2D(3, (32, 64))
    with pytest.raises(NotImplementedError, match="1..8"):
        Discriminator2D(9, (32,))
    with pytest.raises(NotImplementedError):
        Discriminator2D(3, (288, 288))
