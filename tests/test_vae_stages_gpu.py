"""The VAE's training kernels stage by stage (autoregressive_diffusion_amd/vae_train.py Res, Down, Up, Out; csrc/vae_conv3.h,
vae.hip, vae_encoder.hip, vae_train.hip) against the restatement's formulas in float64 (tests/vae_stage_oracle.py): ragged
channel counts in every kernel instantiation, group sizes up to 8, T = g, every (time, spatial) compression pair, and partial
slabs that receive more than one work item; then whole models at the shapes of fixture G17 (training step, inference whole and
streamed through the cache, frames).

A stage's operands are packed by vae.py itself: _pack_res on a seeded ResBlock, and for the 1x1 stages the first block of
VAE._pack_encoder / VAE._pack of the smallest VAE that holds the stage.  Input and emb are leaves, so dx and demb are compared
like the parameter gradients.  Each tensor is held to two metrics against the float64 oracle, rel L2 and max |diff| / rms, each
bounded by 5 x the float32 oracle's own worst figure over the case's tensors of the same kind (outputs / gradients), rel L2
never looser than the whole-model bounds: the bound comes from the oracle, not from the kernels.  profiles/vae_stage_tests.txt
has the measured figures."""
import numpy as np
import pytest
import torch

import vae_cpu_restatement as R
import vae_encoder_cpu_restatement as RE
import vae_stage_oracle as SO
import vae_train_cpu_restatement as RT
from test_vae import rel
from test_vae_gpu import _frames_match
from test_vae_train import g17, g17_restatement64
from test_vae_train_gpu import step_against_the_restatement

DEV = "cuda"
pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))
_CACHE = {}


def _slab_policy(monkeypatch, policy):
    """Installs a slab policy and returns the (work, slabs) of every launch under it: "product", vae_train._nslab itself, or
    "three", at most three slabs, on which every launch with more than three work items takes the second trip of its
    `item += nslab` loop and adds into a slab that is no longer zero."""
    from autoregressive_diffusion_amd import vae_train
    product, calls = vae_train._nslab, []

    def nslab(work, size):
        n = product(work, size) if policy == "product" else min(work, 3)
        calls.append((work, n))
        return n
    monkeypatch.setattr(vae_train, "_nslab", nslab)
    return calls


@pytest.fixture(params=["product", "three"])
def slabs(request, monkeypatch):
    return request.param, _slab_policy(monkeypatch, request.param)


def _cl(x):
    """channels-first (B, C, T, H, W) on the CPU -> a contiguous channels-last leaf on the GPU."""
    return x.permute(0, 2, 3, 4, 1).contiguous().to(DEV).requires_grad_()


def _cf(x):
    return x.permute(0, 4, 1, 2, 3)


def _backward(outs):
    sum((o * RT.cotangents(o.shape, phi, torch.float32).to(DEV)).sum() for o, phi in zip(outs.values(), RT.PHIS)).backward()


def _res_refs(name, case):
    if name not in _CACHE:
        rb, x, emb = SO.res_operands(case)
        g = case[5]
        _CACHE[name] = (rb, x, emb, SO.res_oracle(rb, x, emb, g, torch.float64), SO.res_oracle(rb, x, emb, g, torch.float32))
    return _CACHE[name]


def _run_res(name, case, want, policy, calls):
    from autoregressive_diffusion_amd.vae import _gpt, _nch, _pack_res
    from autoregressive_diffusion_amd.vae_train import Res
    B, T, H, W, C, g, _ = case
    assert (_nch(C), _gpt(C, g)) == want
    rb, x, emb, ref64, ref32 = _res_refs(name, case)
    rb = rb.to(DEV)
    rb.zero_grad(set_to_none=True)
    pk = _pack_res(rb, C, g, dict(device=DEV, dtype=torch.float32))
    bk = dict(g=g, nch=_nch(C), gpt=_gpt(C, g))
    xg = _cl(x)
    eg = None if emb is None else emb.to(DEV).requires_grad_()
    out = Res.apply(xg, eg, rb.conv3d0.conv3d.weight, rb.conv3d0.conv3d.bias, rb.conv3d1.weight, rb.conv3d1.bias, bk, pk)
    assert out.shape == (B, T, H, W, C) and out.is_contiguous()
    outs = dict(out=_cf(out))
    _backward(outs)
    grads = dict(dx=_cf(xg.grad), dwa=rb.conv3d0.conv3d.weight.grad, dba=rb.conv3d0.conv3d.bias.grad, dwb=rb.conv3d1.weight.grad,
                 dbb=rb.conv3d1.bias.grad)
    if eg is not None:
        grads["demb"] = eg.grad
    tiles = -(-H // 16) * -(-W // 16)
    assert calls[0][0] == B * T * tiles and calls[1][0] == B * (T // g) * tiles and len(calls) == 2   # conv B's wgrad, conv A's
    in_order = None
    if "dbb" in SO.KERNEL_ORDER.get(name, ()):               # see SO.KERNEL_ORDER: the one sum replayed in the kernel's order
        in_order = dict(dbb=SO.bias_grad_in_kernel_order(RT.cotangents((B, C, T, H, W), RT.PHIS[0], torch.float32), calls[0][1]))
    bad = SO.compare(f"res {name} {case} {policy}:", (outs, grads), ref64, ref32, in_order)
    assert not bad, "\n".join(bad)
    return calls


@pytest.mark.parametrize("name", list(SO.RES_CASES))
def test_res_stage(name, slabs):
    """Res: out, dx, demb, dwa, dba, dwb, dbb against float64 at the twelve cases of SO.RES_CASES, on both slab policies; on
    three slabs r02, r05 and r06 (8, 36 and 4 work items for conv A) must wrap."""
    policy, calls = slabs
    case, want = SO.RES_CASES[name]
    _run_res(name, case, want, policy, calls)
    if policy == "three" and name in SO.RES_WRAP_WORK:
        assert (SO.RES_WRAP_WORK[name], 3) in calls and all(w > n for w, n in calls)


def test_res_stage_where_the_1024_cap_binds(monkeypatch):
    """Res (1, 9, 176, 176, 4, 1): 121 tiles x 9 frames = 1089 work items on the product's own 1024 slabs, so 65 slabs receive
    two items; held to the same bounds as every other case."""
    case, want = SO.RES_CAP_CASE
    B, T, H, W, C, g, _ = case
    work = B * (T // g) * -(-H // 16) * -(-W // 16)
    assert work > 1024
    calls = _run_res("cap", case, want, "product", _slab_policy(monkeypatch, "product"))
    assert calls == [(work, 1024), (work, 1024)]


def _lin_refs(kind, name):
    if name not in _CACHE:
        vae, conv, x, tc, sc, lvm = SO.lin_operands(kind, name)
        refs = [SO.lin_oracle(kind, x, conv.weight, conv.bias, tc, sc, dt, lvm=lvm) for dt in (torch.float64, torch.float32)]
        _CACHE[name] = (vae.to(DEV), conv, x, refs[0], refs[1])
    return _CACHE[name]


def _check_lin(kind, p, grid, outs, grads, ref64, ref32, policy, calls, name):
    K, N = SO.lin_kn(kind, p)
    rows, rpc = int(np.prod(grid)), SO.lin_rpc(K, N)
    assert rows % rpc != 0
    bad = SO.compare(f"{kind} {name} {p} grid {grid} {policy}:", (outs, grads), ref64, ref32)
    assert not bad, "\n".join(bad)
    assert [w for w, _ in calls] == [-(-rows // rpc)]
    if policy == "three" and name in SO.LIN_WRAP:
        assert calls[0][0] > 3 and calls[0][1] == 3


@pytest.mark.parametrize("name", list(SO.DOWN_CASES))
def test_down_stage(name, slabs):
    """Down: y, dx, dw, db against float64: a permuted channels-first view (block 0), the vectorised load with the ragged
    store, Cin not a multiple of 4, windows of length 1, K = 512."""
    from autoregressive_diffusion_amd.vae_train import Down
    policy, calls = slabs
    p, grid, permuted = SO.DOWN_CASES[name]
    vae, conv, x, ref64, ref32 = _lin_refs("down", name)
    vae.zero_grad(set_to_none=True)
    bk = vae._pack_encoder(torch.device(DEV))["blocks"][0]
    assert (bk["Cin"], bk["tc"], bk["sc"], bk["C"]) == p
    xg = x.to(DEV).requires_grad_() if permuted else _cl(x)
    xin = xg.permute(0, 2, 3, 4, 1) if permuted else xg
    assert xin.is_contiguous() != permuted
    y = Down.apply(xin, conv.weight, conv.bias, bk)
    assert y.shape == grid + (p[3],)
    outs = dict(y=_cf(y))
    _backward(outs)
    grads = dict(dx=xg.grad if permuted else _cf(xg.grad), dw=conv.weight.grad, db=conv.bias.grad)
    _check_lin("down", p, grid, outs, grads, ref64, ref32, policy, calls, name)


@pytest.mark.parametrize("name", list(SO.UP_CASES))
def test_up_stage(name, slabs):
    """Up: y, dx, dw, db against float64 at every (tc, sc) pair, from a permuted view and at full width."""
    from autoregressive_diffusion_amd.vae_train import Up
    policy, calls = slabs
    p, grid, permuted = SO.UP_CASES[name]
    vae, conv, x, ref64, ref32 = _lin_refs("up", name)
    vae.zero_grad(set_to_none=True)
    bk = vae._pack(torch.device(DEV))["blocks"][0]
    assert (bk["C"], bk["tc"], bk["sc"]) == p
    xg = x.to(DEV).requires_grad_() if permuted else _cl(x)
    xin = xg.permute(0, 2, 3, 4, 1) if permuted else xg
    assert xin.is_contiguous() != permuted
    y = Up.apply(xin, conv.weight, conv.bias, bk)
    B, T, H, W = grid
    assert y.shape == (B, T * p[1], H * p[2], W * p[2], p[0])
    outs = dict(y=_cf(y))
    _backward(outs)
    grads = dict(dx=xg.grad if permuted else _cf(xg.grad), dw=conv.weight.grad, db=conv.bias.grad)
    _check_lin("up", p, grid, outs, grads, ref64, ref32, policy, calls, name)


@pytest.mark.parametrize("name", list(SO.OUT_CASES))
def test_out_stage(name, slabs):
    """Out: y, dx, dw, db against float64, and for the last block (mean, logvar) with d logvar_multiplier at -1.7."""
    from autoregressive_diffusion_amd.vae_train import Out
    policy, calls = slabs
    p, grid, last = SO.OUT_CASES[name]
    vae, conv, x, ref64, ref32 = _lin_refs("out", name)
    vae.zero_grad(set_to_none=True)
    dpk = vae._pack(torch.device(DEV))
    bk = dpk["blocks"][0]
    assert (bk["C"], bk["Cout"]) == p
    xg = _cl(x)
    if last:
        lvm = vae.decoder.logvar_multiplier
        assert float(lvm.detach()) == pytest.approx(-1.7)
        mean, logvar = Out.apply(xg, conv.weight, conv.bias, lvm, bk, dpk["lvm"])
        outs = dict(mean=mean, logvar=logvar)
    else:
        outs = dict(y=_cf(Out.apply(xg, conv.weight, conv.bias, None, bk, None)))
    _backward(outs)
    grads = dict(dx=_cf(xg.grad), dw=conv.weight.grad, db=conv.bias.grad)
    if last:
        grads["dlvm"] = lvm.grad
    _check_lin("out", p, grid, outs, grads, ref64, ref32, policy, calls, name)


# ---- whole models at the shapes of fixture G17
def _g17_vae(config):
    from autoregressive_diffusion_amd.vae import VAE
    _, x, ts, noise, sd, kw = g17(config)
    C = kw["channels"][-1]
    kw = dict(kw, mean=torch.linspace(-0.3, 0.4, C).tolist(), std=torch.linspace(0.8, 1.3, C).tolist())
    vae = VAE(**kw)
    vae.load_state_dict(sd, strict=True)
    return vae.to(DEV), x, ts, noise, sd, kw


@pytest.mark.parametrize("config", ["A", "B"])
def test_training_step_at_g17_shapes(config):
    """Config A (group sizes 8 / 4 / 2, compression pairs (2,2) and (2,1)) and B (pairs (1,2) and (2,1), widths 48 / 6 / 20):
    outputs and every parameter gradient of a training step against the restatement in float64, which fixture G17 pins to the
    reference at these shapes; mean bit for bit what encode gives."""
    vae, x, ts, noise, _, _ = _g17_vae(config)
    step_against_the_restatement(vae.train(), x, ts, noise, f"G17 {config}", ref=g17_restatement64(config))


def _encoder_chunk(kw):
    """The fewest frames the encoder takes at once: every block sees a multiple of its group size."""
    tcs = kw["time_compressions"]
    groups = [int(g) for g in np.cumprod(tcs)[::-1]]
    n = int(np.prod(tcs))
    while any((n // int(np.prod(tcs[:i + 1]))) % g for i, g in enumerate(groups)):
        n += int(np.prod(tcs))
    return n


@pytest.mark.parametrize("config", ["A", "B"])
def test_inference_at_g17_shapes(config):
    """encode and decode of the same models against the encoder and decoder restatements within rel L2 1e-5: the whole
    sequence, and streamed through the cache in the smallest chunks the model takes (decoder: one latent frame; encoder: one
    latent frame for B, two for A, whose first block has g = 8 on frames at half rate -- there over a sequence twice as long),
    the restatements carrying their own caches.  decode_frames against the restatement's frames before truncation."""
    vae, x, ts, noise, sd, kw = _g17_vae(config)
    vae = vae.eval()
    B = x.shape[0]
    mean, _ = vae.encode(x.to(DEV))
    rm, _ = RE.encode(sd, kw, x)
    print(f"G17 {config}: encode {rel(mean.cpu(), rm):.2e}")
    assert mean.shape == rm.shape and rel(mean.cpu(), rm) <= 1e-5
    n = _encoder_chunk(kw)
    assert n == {"A": 16, "B": 2}[config]
    xs = x if x.shape[2] > n else torch.cat((x, torch.rand(x.shape, generator=torch.Generator().manual_seed(1720)) * 2 - 1), dim=2)
    ms, rs, c, rc = [], [], None, None
    for s in range(0, xs.shape[2], n):
        m, c = vae.encode(xs[:, :, s:s + n].to(DEV), c)
        r, rc = RE.encode(sd, kw, xs[:, :, s:s + n], rc)
        ms.append(m.cpu())
        rs.append(r)
    assert len(ms) >= 2
    print(f"G17 {config}: encode in chunks of {n} frames {rel(torch.cat(ms, dim=2), torch.cat(rs, dim=2)):.2e}")
    assert rel(torch.cat(ms, dim=2), torch.cat(rs, dim=2)) <= 1e-5
    z = rm + 0.5 * noise
    t = torch.tensor([0.1, 0.35])[:B]
    dm, dl, _ = vae.decode(z.to(DEV), t.to(DEV))
    qm, ql, _ = R.decode(sd, kw, z, t)
    print(f"G17 {config}: decode {rel(dm.cpu(), qm):.2e} {rel(dl.cpu(), ql):.2e}")
    assert dm.shape == qm.shape == x.shape and rel(dm.cpu(), qm) <= 1e-5 and rel(dl.cpu(), ql) <= 1e-5
    ms, ls, qs, qls, c, rc = [], [], [], [], None, None
    for s in range(z.shape[2]):
        m, lv, c = vae.decode(z[:, :, s:s + 1].to(DEV), t.to(DEV), c)
        q, qv, rc = R.decode(sd, kw, z[:, :, s:s + 1], t, rc)
        ms.append(m.cpu()); ls.append(lv.cpu()); qs.append(q); qls.append(qv)
    assert len(ms) == 2
    print(f"G17 {config}: decode latent frame by latent frame {rel(torch.cat(ms, dim=2), torch.cat(qs, dim=2)):.2e} "
          f"{rel(torch.cat(ls, dim=2), torch.cat(qls, dim=2)):.2e}")
    assert rel(torch.cat(ms, dim=2), torch.cat(qs, dim=2)) <= 1e-5 and rel(torch.cat(ls, dim=2), torch.cat(qls, dim=2)) <= 1e-5
    latents = noise.permute(0, 2, 1, 3, 4).contiguous()
    frames, _ = vae.decode_frames(latents.to(DEV))
    pre = R.frames_pre(sd, kw, latents)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == tuple(pre.shape)
    bad, off = _frames_match(frames.cpu(), pre)
    print(f"G17 {config}: decode_frames: {bad} bad, {off} one level off of {frames.numel()}")
    assert bad == 0
