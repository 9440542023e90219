"""CPU checks of VAE training (autoregressive_diffusion_amd/vae.py VAE.forward, vae_train.py): the training restatement against
fixture G16 (the reference's float64 outputs and parameter gradients) and fixture G17 (the same at group size 8 and at every
compression pair), the refusals of `forward`, the data-gradient weight layouts of the two ResBlock convs against autograd, the
slab policy, and the comparator of the stage tests (tests/vae_stage_oracle.py) against the restatement with one defect at a
time.  No kernel is launched."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vae_stage_oracle as SO
import vae_train_cpu_restatement as RT
from test_vae_encoder import g15

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel64(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).norm() / b.norm()).item()


def g16():
    """(outputs and draws, parameter gradients, ref32_rel per parameter, x, state dict, kwargs) of fixture G16."""
    z = np.load(os.path.join(G, "g16_vae_train.npz"), allow_pickle=False)
    zg = np.load(os.path.join(G, "g16_vae_train_grads.npz"), allow_pickle=False)
    _, _, x, sd, kw = g15()
    grads = {k: torch.from_numpy(zg[k]) for k in zg.files if not k.startswith("ref32_rel/")}
    ref32 = {k[len("ref32_rel/"):]: float(zg[k]) for k in zg.files if k.startswith("ref32_rel/")}
    return z, grads, ref32, x, sd, kw


_REF = {}


def g16_restatement64():
    """The restatement's float64 run on G16's inputs, computed once and shared."""
    if not _REF:
        z, _, _, x, sd, kw = g16()
        _REF["v"] = RT.grads(sd, kw, x, torch.from_numpy(z["t_sample"]), torch.from_numpy(z["noise"]))
    return _REF["v"]


def test_restatement_against_g16():
    """The restatement in float64 reproduces the reference's float64 outputs and every one of its 174 767 parameter gradients to
    rel L2 1e-6 (the fixture is stored as float32: rounding alone gives about 3e-8)."""
    z, grads, ref32, x, sd, kw = g16()
    assert x.shape == (2, 3, 12, 24, 40) and z["noise"].shape == (2, 8, 3, 6, 10) and z["t_sample"].shape == (2,)
    assert sum(v.numel() for v in grads.values()) == 174767 and set(ref32) == set(grads)
    assert set(grads) == {k for k in sd if "fourier_cond" not in k}
    outs, g = g16_restatement64()
    for k in ("mean", "r_mean", "r_logvar"):
        print(f"restatement vs G16: {k} {rel64(outs[k], z[k]):.2e}")
        assert rel64(outs[k], z[k]) <= 1e-6, k
    worst = max(grads, key=lambda k: rel64(g[k], grads[k]))
    print(f"restatement vs G16: worst gradient {worst} {rel64(g[worst], grads[worst]):.2e}")
    for k in grads:
        assert rel64(g[k], grads[k]) <= 1e-6, k
    print("reference float32 vs float64, worst:", max(ref32, key=ref32.get), max(ref32.values()))


def test_forward_refusals():
    """`forward` on a CPU-resident model or a CPU input keeps pointing to the reference's edm2.vae; bad shapes (frames, t_sample,
    noise) raise ValueError first."""
    from autoregressive_diffusion_amd.vae import VAE
    vae = VAE(channels=[3, 8, 8, 8], n_res_blocks=1)
    x = torch.zeros(1, 3, 4, 16, 16)
    for kw in ({}, dict(t_sample=torch.zeros(1), noise=torch.zeros(1, 8, 1, 4, 4))):
        with pytest.raises(NotImplementedError, match="edm2.vae"):
            vae(x, **kw)
    vae.eval()
    with pytest.raises(NotImplementedError, match="edm2.vae"):
        vae(x)
    for shape in ((1, 3, 6, 16, 16), (1, 3, 4, 18, 16), (1, 3, 4, 16, 14), (3, 4, 16, 16), (1, 4, 4, 16, 16), (1, 3, 0, 16, 16)):
        with pytest.raises(ValueError):
            vae(torch.zeros(shape))
    with pytest.raises(ValueError, match="t_sample"):
        vae(x, t_sample=torch.zeros(2))
    with pytest.raises(ValueError, match="noise"):
        vae(x, noise=torch.zeros(1, 8, 1, 4, 5))


@pytest.mark.parametrize("C,g", [(8, 4), (16, 2), (5, 1), (3, 2)])
def test_dgrad_weight_layouts_against_autograd(C, g):
    """vae_train._pack_dgrad: the packed data-gradient weights of conv A (mirrored causality: 2g frames of da, the own group and
    the next one, zero beyond the end) and of conv B, applied as include/oniris.h states them, give autograd's gradient of the
    two convs with the detached prefix."""
    from autoregressive_diffusion_amd.vae import _gpt, _nch
    from autoregressive_diffusion_amd.vae_train import _pack_dgrad
    gen = torch.Generator().manual_seed(C * 10 + g)
    B, T, H, W = 2, 3 * g, 5, 4
    wa = torch.randn(C * g, C, 2 * g, 3, 3, generator=gen, dtype=torch.float64)
    wb = torch.randn(C, C, 1, 3, 3, generator=gen, dtype=torch.float64)
    y = torch.randn(B, C, T, H, W, generator=gen, dtype=torch.float64, requires_grad=True)
    yp = F.pad(y, (1, 1, 1, 1))
    a = F.conv3d(torch.cat((yp[:, :, :g].detach(), yp), dim=2), wa, None, stride=(g, 1, 1))
    a = a.reshape(B, C, g, T // g, H, W).permute(0, 1, 3, 2, 4, 5).reshape(B, C, T, H, W)
    da = torch.randn(B, C, T, H, W, generator=gen, dtype=torch.float64)
    (dy,) = torch.autograd.grad(a, y, da)
    wda, wdb = _pack_dgrad(wa, wb, C, g)
    nch, gpt = _nch(C), _gpt(C, g)
    assert wda.shape == (g // gpt, 2 * g, 3, 3, C, nch, gpt) and wdb.shape == (3, 3, C, nch)
    dap = F.pad(torch.cat((da, torch.zeros(B, C, g, H, W, dtype=torch.float64)), dim=2), (1, 1, 1, 1)).float()
    got = torch.zeros(B, C, T, H, W)
    for q in range(T // g):
        for r in range(g):
            for j in range(2 * g):
                for ky in range(3):
                    for kx in range(3):
                        w = wda[r // gpt, j, ky, kx, :, :C, r % gpt]                   # c, ci
                        got[:, :, q * g + r] += torch.einsum("bchw,ci->bihw", dap[:, :, q * g + j, ky:ky + H, kx:kx + W], w)
    assert rel64(got, dy) <= 1e-6
    assert float(wda[..., C:, :].abs().sum()) == 0 and float(wdb[..., C:].abs().sum()) == 0
    u = torch.randn(B, C, T, H, W, generator=gen, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(B, C, T, H, W, generator=gen, dtype=torch.float64)
    (du,) = torch.autograd.grad(F.conv3d(u, wb, None, padding=(0, 1, 1)), u, dout)
    dop = F.pad(dout, (1, 1, 1, 1)).float()
    got = torch.zeros(B, C, T, H, W)
    for ky in range(3):
        for kx in range(3):
            got += torch.einsum("bcthw,ci->bithw", dop[:, :, :, ky:ky + H, kx:kx + W], wdb[ky, kx, :, :C])
    assert rel64(got, du) <= 1e-6


def g17(config):
    """(fixture entries of config "A" / "B" by name, x, t_sample, noise, the regenerated state dict, kwargs) of fixture G17."""
    z = np.load(os.path.join(G, "g17_vae_shapes.npz"), allow_pickle=False)
    p = config + "/"
    e = {k[len(p):]: z[k] for k in z.files if k.startswith(p)}
    shapes = [tuple(int(v) for v in s.split(",")) if s else () for s in e["shapes"].tolist()]
    sd = SO.seeded_state_dict(e["names"].tolist(), shapes, int(e["seed"]))
    kw = dict(channels=e["kw_channels"].tolist(), n_res_blocks=int(e["kw_n_res_blocks"]),
              time_compressions=e["kw_time_compressions"].tolist(), spatial_compressions=e["kw_spatial_compressions"].tolist())
    return e, torch.from_numpy(e["x"]), torch.from_numpy(e["t_sample"]), torch.from_numpy(e["noise"]), sd, kw


_REF17 = {}


def g17_restatement64(config):
    """The restatement's float64 run on G17's inputs, computed once per config and shared."""
    if config not in _REF17:
        _, x, ts, noise, sd, kw = g17(config)
        _REF17[config] = RT.grads(sd, kw, x, ts, noise)
    return _REF17[config]


@pytest.mark.parametrize("config", ["A", "B"])
def test_restatement_against_g17(config):
    """The restatement in float64 reproduces the reference's float64 run at time_compressions [2,2,2] / spatial [2,1,2] (A) and
    [1,1,2] / [2,2,1] (B) to 1e-9 relative (measured 5e-15: room for another BLAS summation order, nothing else): the three
    outputs element by element and, of every parameter gradient, the L2 norm and the projection on cos(0.3 i + 1), the latter
    relative to the norm times sqrt(n / 2), the projection's own scale.  The fixture's parameters are regenerated from its seed."""
    e, x, ts, noise, sd, kw = g17(config)
    from autoregressive_diffusion_amd.vae import VAE
    mine = VAE(**kw).state_dict()
    assert list(mine) == list(sd) and all(mine[k].shape == sd[k].shape for k in sd)
    outs, g = g17_restatement64(config)
    for k in ("mean", "r_mean", "r_logvar"):
        assert e[k].dtype == np.float64
        print(f"restatement vs G17 {config}: {k} {rel64(outs[k], e[k]):.2e}")
        assert rel64(outs[k], e[k]) <= 1e-9, k
    names = {k[len("gnorm/"):] for k in e if k.startswith("gnorm/")}
    assert names == set(g) == {k for k in sd if "fourier_cond" not in k}
    worst = 0.0
    for k in sorted(names):
        v = g[k].double().reshape(-1)
        n, norm = v.numel(), float(e["gnorm/" + k])
        assert norm > 0, k
        proj = float((v * torch.cos(0.3 * torch.arange(n, dtype=torch.float64) + 1)).sum())
        en = abs(float(v.norm()) - norm) / norm
        ep = abs(proj - float(e["gproj/" + k])) / (norm * max(1.0, (n / 2) ** 0.5))
        worst = max(worst, en, ep)
        assert en <= 1e-9 and ep <= 1e-9, (k, en, ep)
    print(f"restatement vs G17 {config}: worst gradient norm / projection {worst:.2e}")
    print("reference float32 vs float64, worst:", max(float(e[k]) for k in e if k.startswith("ref32_rel/")))
    assert max(float(e[k]) for k in e if k.startswith("ref32_rel/")) <= 1.0e-5          # the basis of GRAD_TOL holds here too


def test_nslab_properties():
    """vae_train._nslab over a grid of (work, size): between 1 and min(work, 1024) slabs, and never more memory than _SLAB_BYTES
    unless 64 slabs alone take more."""
    from autoregressive_diffusion_amd.vae_train import _SLAB_BYTES, _nslab
    works = [1, 2, 3, 63, 64, 65, 1000, 1023, 1024, 1025, 1089, 5000, 10 ** 6, 2 ** 31 - 1]
    sizes = [1, 5, 148, 292, 9 * 64 * 64 + 64, 16383, 16384, 16385, 2 * 64 * 9 * 64 * 64 + 8 * 64, 262143, 262144, 262145,
             (1 << 24) - 1, 1 << 24, (1 << 24) + 1, 1 << 28]
    for work in works:
        for size in sizes:
            n = _nslab(work, size)
            assert isinstance(n, int) and 1 <= n <= min(work, 1024), (work, size, n)
            assert n * size * 4 <= max(_SLAB_BYTES, 64 * size * 4), (work, size, n)
    assert _nslab(1089, 292) == 1024 and _nslab(5000, 9 * 64 * 64 + 64) == (64 << 20) // (4 * 36928) and _nslab(5000, 1 << 20) == 64


_STAGE = {}


def _res_stage(name):
    """Operands and the float64 / float32 oracle of a Res case, computed once."""
    if name not in _STAGE:
        case = SO.RES_CASES[name][0]
        rb, x, emb = SO.res_operands(case)
        _STAGE[name] = (rb, x, emb, case[5], SO.res_oracle(rb, x, emb, case[5], torch.float64),
                        SO.res_oracle(rb, x, emb, case[5], torch.float32))
    return _STAGE[name]


def _lin_stage(kind, name):
    if name not in _STAGE:
        _, conv, x, tc, sc, lvm = SO.lin_operands(kind, name)
        _STAGE[name] = (x, conv, tc, sc, SO.lin_oracle(kind, x, conv.weight, conv.bias, tc, sc, torch.float64, lvm=lvm),
                        SO.lin_oracle(kind, x, conv.weight, conv.bias, tc, sc, torch.float32, lvm=lvm))
    return _STAGE[name]


def _moved(what, mutant, ref64, ref32):
    """The largest ratio, over the compared tensors and both metrics, of a defective oracle's distance from the float64 oracle
    to the bound the stage test holds that tensor to."""
    bnd, _ = SO.bounds(ref64, ref32)
    best = 0.0
    for m, r64, (brel, bmax) in zip(mutant, ref64, bnd):
        for k in r64:
            rel, mx = SO.metrics(m[k], r64[k])
            best = max(best, rel / brel, mx / bmax)
    print(f"{what}: moved a compared tensor by {best:.1e} x its bound")
    return best


@pytest.mark.parametrize("name", ["r02", "r06"])
def test_stage_comparator_sees_res_defects(name):
    """The Res stage comparison would fail on each of: the prefix not detached, a zero prefix, the last halo column of a tile
    dropped, the group interleave '(c g) t -> c (t g)' transposed -- each moves a compared tensor by at least 100 x its bound.
    Without a defect the rewritten block IS the restatement's (bit for bit), so each defect is the only difference."""
    rb, x, emb, g, ref64, ref32 = _res_stage(name)
    same = SO.res_oracle(rb, x, emb, g, torch.float64, SO.res_block_defect(None))
    assert all(torch.equal(a[k], b[k]) for a, b in zip(same, ref64) for k in b)
    for defect in SO.RES_DEFECTS:
        mutant = SO.res_oracle(rb, x, emb, g, torch.float64, SO.res_block_defect(defect))
        assert _moved(f"{name} {defect}", mutant, ref64, ref32) >= 100, defect


@pytest.mark.parametrize("kind,name,defects", [("down", "d1", ("hc_wc", "area_floor")), ("up", "u0", ("hc_wc",)),
                                               ("out", "o1", ("area_floor",))])
def test_stage_comparator_sees_lin_defects(kind, name, defects):
    """The 1x1 stage comparisons would fail on hc / wc swapped in the patch rearrangement (sc = 2, H != W) and on an area window
    whose upper end is taken with floor: each moves a compared tensor by at least 100 x its bound."""
    x, conv, tc, sc, ref64, ref32 = _lin_stage(kind, name)
    same = SO.lin_oracle(kind, x, conv.weight, conv.bias, tc, sc, torch.float64, fn=SO.lin_defect(kind, None))
    assert all(torch.equal(a[k], b[k]) for a, b in zip(same, ref64) for k in b)
    for defect in defects:
        mutant = SO.lin_oracle(kind, x, conv.weight, conv.bias, tc, sc, torch.float64, fn=SO.lin_defect(kind, defect))
        assert _moved(f"{name} {defect}", mutant, ref64, ref32) >= 100, defect


def test_stage_cases_are_what_they_claim():
    """Every Res case reaches the (NCH, GPT) it is listed for, the wrap cases have the stated work-item counts, every case lies
    inside the entry points' domain (C <= 64, T a multiple of g, K <= 512, dynamic LDS <= 160 KiB) and no 1x1 grid's row count
    is a multiple of the rows per chunk."""
    from autoregressive_diffusion_amd.vae import _gpt, _nch
    for name, (case, want) in list(SO.RES_CASES.items()) + [("cap", SO.RES_CAP_CASE)]:
        B, T, H, W, C, g, _ = case
        assert (_nch(C), _gpt(C, g)) == want, name
        assert 1 <= C <= 64 and T % g == 0 and T >= g and g % _gpt(C, g) == 0, name
        tile = 18 * 18 * (C | 1) * 4
        nacc = _nch(C) * _gpt(C, g)
        rows = 3 if tile + 9 * C * nacc * 4 <= 64 * 1024 else 1
        assert tile + rows * 3 * C * nacc * 4 <= 160 * 1024 and tile + 256 * C * 4 <= 160 * 1024, name
        if name in SO.RES_WRAP_WORK:
            assert B * (T // g) * -(-H // 16) * -(-W // 16) == SO.RES_WRAP_WORK[name], name
    B, T, H, W, C, g, _ = SO.RES_CAP_CASE[0]
    assert B * (T // g) * -(-H // 16) * -(-W // 16) == 1089 and B * T * H * W * C <= 1.2e6
    small = 0
    for kind, cases in (("down", SO.DOWN_CASES), ("up", SO.UP_CASES), ("out", SO.OUT_CASES)):
        for name, (p, grid, _) in cases.items():
            K, N = SO.lin_kn(kind, p)
            rows, rpc = int(np.prod(grid)), SO.lin_rpc(K, N)
            assert K <= 512 and N <= 512 and max(p[0], p[-1] if kind != "up" else p[0]) <= 64, name
            assert rpc * (K + 1 + N) * 4 <= 64 * 1024 and rows % rpc != 0, (name, rows, rpc)
            small += rows < rpc
            if name in SO.LIN_WRAP:
                assert -(-rows // rpc) > 3, name
    assert small >= 1


def test_bias_grad_replay_is_a_sum():
    """SO.bias_grad_in_kernel_order (the float32 replay of vt_wgrad3_kernel's bias-gradient order that r06's dbb is held to):
    on ragged tiles and any slab count it is the sum over (b, t, h, w) -- float32 rounding away from the float64 sum, and
    exactly it on integers."""
    gen = torch.Generator().manual_seed(1730)
    d = torch.randn(2, 5, 3, 17, 33, generator=gen)
    ints = torch.randint(-8, 9, d.shape, generator=gen).float()
    for nslab in (1, 3, 7, 36, 1024):
        got = SO.bias_grad_in_kernel_order(d, nslab)
        assert got.dtype == torch.float32 and rel64(got, d.double().sum(dim=(0, 2, 3, 4))) <= 1e-5
        assert torch.equal(SO.bias_grad_in_kernel_order(ints, nslab), ints.sum(dim=(0, 2, 3, 4)))
