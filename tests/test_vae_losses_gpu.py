"""The VAE losses on HIP kernels (autoregressive_diffusion_amd/vae_losses.py, csrc/vae_loss.hip) against fixture G21 (the
reference's float64 run), against the float64 restatement (tests/vae_losses_cpu_restatement.py), against themselves (fused against
single calls, two runs) and inside one VAE training step.  Every compared figure is printed (-s); profiles/vae_losses_tests.txt is
that output.

Bounds (from the summation rule of csrc/vae_loss.hip, not from the kernels' results):
  losses            |loss - ref64| <= 1e-5 mean|term|: at most 64 terms in a row, then trees of depth <= 40 -> 104 x 2^-24 = 6.2e-6 on the
                    sum; the elementwise roundings (a 2-ulp expf among them) stay below 1e-6
  fused gradients   rel L2 against float64 <= 2e-6: at most 16 roundings of 2^-24 on an element
  worst-k gradient  the same set of nonzero elements; |g - g64| <= 5e-7 |g64| elementwise: only the order of three products differs
  selection         threshold bits and both counts exactly"""
import contextlib

import numpy as np
import pytest
import torch

import vae_losses_cpu_restatement as R
import vae_losses_gen as G
from test_vae_losses import LOSSES, fused64, g21, rel

DEV = "cuda"
pytestmark = pytest.mark.gpu
LOSS_TOL, FUSED_GRAD_TOL, WK_GRAD_TOL = 1e-5, 2e-6, 5e-7
VARIANTS = ("contiguous", "channels_last", "wrap", "wrap_channels_last")


@contextlib.contextmanager
def max_blocks(n):
    from autoregressive_diffusion_amd import vae_losses as V
    old, V._MAX_BLOCKS = V._MAX_BLOCKS, n
    try:
        yield
    finally:
        V._MAX_BLOCKS = old


def variant_ctx(variant):
    return max_blocks(3) if variant.startswith("wrap") else contextlib.nullcontext()


def channels_last(t):
    """The scripts' frames: stored (b, t, h, w, c), handed over as the permuted view (b, c, t, h, w)."""
    return t.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)


def operands(case, variant, grad=True):
    m, lv, tg = (t.to(DEV) for t in G.inputs(case))
    if variant.endswith("channels_last"):
        tg = channels_last(tg)
        assert not tg.is_contiguous()
    return tuple(t.requires_grad_(grad) for t in (m, lv, tg))


def close(a, b, tol, scale=None):
    """|a - b| <= tol * scale (scale: |b| by default), or both the same infinity / both NaN."""
    a, b = float(a), float(b)
    if np.isnan(b) or np.isinf(b):
        return (np.isnan(a) and np.isnan(b)) or a == b
    return abs(a - b) <= tol * (abs(b) if scale is None else scale)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", list(G.CASES))
def test_fused_losses_against_float64(case, variant):
    from autoregressive_diffusion_amd import vae_losses as V
    z = g21()
    want_losses, termabs, want_grads = fused64(case)
    m, lv, tg = operands(case, variant)
    with variant_ctx(variant):
        trio = V.recon_losses(m, lv, tg)
        sum(c * v for c, v in zip(G.COTS, trio)).backward()
    for name, got, want, ta in zip(LOSSES, trio, want_losses, termabs):
        assert got.dim() == 0 and got.dtype == torch.float32 and got.grad_fn is not None
        assert abs(want - float(z[f"{case}/{name}"])) <= 1e-12 * abs(want)
        err = abs(got.item() - want) / ta
        print(f"{case} {variant}: {name} {got.item():.8f} ref64 {want:.8f} |diff| / mean|term| {err:.2e} (bound {LOSS_TOL:.0e}; "
              f"reference fp32 {float(z[f'{case}/ref32_rel/{name}']):.1e})")
        assert err <= LOSS_TOL, name
    for name, got, want in zip(("dmean", "dlogvar", "dtarget"), (m.grad, lv.grad, tg.grad), want_grads):
        assert got.shape == want.shape and got.dtype == torch.float32
        e = rel(got.cpu(), want)
        print(f"{case} {variant}: {name} rel L2 {e:.2e} (bound {FUSED_GRAD_TOL:.0e})")
        assert e <= FUSED_GRAD_TOL, name
    assert torch.equal(tg.grad, -m.grad)


@pytest.mark.selfcheck
@pytest.mark.parametrize("variant", ("contiguous", "wrap_channels_last"))
def test_recon_losses_equal_the_single_calls_bit_for_bit(variant):
    from autoregressive_diffusion_amd import vae_losses as V
    for case in G.CASES:
        m, lv, tg = operands(case, variant)
        with variant_ctx(variant):
            trio = V.recon_losses(m, lv, tg)
            singles = (V.GaussianLoss(m, lv, tg), V.l1_loss(m, tg), V.mse_loss(m, tg))
            for name, a, b in zip(LOSSES, trio, singles):
                print(f"{case} {variant}: {name} fused {a.item():.9g} single {b.item():.9g}")
                assert torch.equal(a, b), name
            for i, name in enumerate(LOSSES):                 # and the gradient of one output alone equals the single call's
                ga = torch.autograd.grad(trio[i], (m, tg), retain_graph=True)
                gb = torch.autograd.grad(singles[i], (m, tg))
                assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1]), name


def _selection(recon, target, k):
    from autoregressive_diffusion_amd import vae_losses as V
    loss, state = V.worst_k_select(recon.detach(), target.detach(), k)
    s = state.cpu().numpy().view(np.uint32)
    return loss, int(s[0]), int(s[1]), int(s[2])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("wk", list(G.WORSTK))
def test_worst_k_against_g21(wk, variant):
    from autoregressive_diffusion_amd import vae_losses as V
    z = g21()
    case, percent = G.WORSTK[wk]
    m, _, tg = operands(case, variant)
    k, want = int(z[f"{wk}/k"]), float(z[f"{wk}/loss"])
    sel = R.select(*[t for i, t in enumerate(G.inputs(case)) if i != 1], k)
    with variant_ctx(variant):
        _, thr, gt, eq = _selection(m, tg, k)
        loss = V.worst_k_percent_loss(m, tg, percent=percent)
        (G.WK_COT * loss).backward()
    print(f"{wk} {variant}: k {k} threshold {thr:#010x} (G21 {int(z[f'{wk}/thr']):#010x}) count_gt {gt} count_eq {eq}; loss {loss.item():.8f} "
          f"ref64 {want:.8f} rel {abs(loss.item() - want) / want:.2e} (bound {LOSS_TOL:.0e})")
    assert (thr, gt, eq) == (int(z[f"{wk}/thr"]), int(z[f"{wk}/count_gt"]), int(z[f"{wk}/count_eq"]))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and abs(loss.item() - want) <= LOSS_TOL * want
    g = m.grad.cpu().double().numpy().ravel()
    g64 = R.worst_k_grad(sel, G.WK_COT)
    if f"{wk}/drecon" in z:                                   # the reference's own gradient, stored for a unit cotangent
        ref = G.WK_COT * z[f"{wk}/drecon"].astype(np.float64).ravel()
        assert np.array_equal(ref != 0, g64 != 0) and np.all(np.abs(ref - g64) <= 2e-7 * np.abs(g64))
    else:
        assert abs(np.linalg.norm(g64) - G.WK_COT * float(z[f"{wk}/norm/drecon"])) <= 2e-7 * np.linalg.norm(g64)
    worst = float(np.max(np.abs(g - g64)[g64 != 0] / np.abs(g64[g64 != 0])))
    print(f"{wk} {variant}: gradient nonzero {int((g != 0).sum())} (k {k}), worst elementwise rel {worst:.2e} (bound {WK_GRAD_TOL:.0e})")
    assert np.array_equal(g != 0, g64 != 0) and int((g != 0).sum()) == int(z[f"{wk}/nonzero"])
    assert np.all(np.abs(g - g64) <= WK_GRAD_TOL * np.abs(g64))
    assert torch.equal(tg.grad, -m.grad)
    if wk == "mid_all":                                       # k = numel: the same number as mse_loss
        with variant_ctx(variant):
            mse = V.mse_loss(m, tg).item()
        print(f"{wk} {variant}: mse_loss {mse:.8f}")
        assert abs(loss.item() - mse) <= 2 * LOSS_TOL * mse
    if wk == "tiny_k1":                                       # k = 1: exactly the maximum
        assert loss.item() == float(sel["e"].max())


@pytest.mark.parametrize("variant", ("contiguous", "strided", "wrap"))
@pytest.mark.parametrize("name", G.CRAFTED)
def test_worst_k_on_crafted_key_sets(name, variant):
    """Threshold bits and both counts exactly as the restatement gives them, the loss against its float64 value, the gradient
    elementwise; ties: every tied element carries (k - count_gt) / count_eq."""
    from autoregressive_diffusion_amd import vae_losses as V
    r0, t0, k = G.crafted(name)
    sel = R.select(r0, t0, k)
    if variant == "strided":                                  # every other element of a buffer twice the size
        buf = torch.zeros(r0.numel() * 2, device=DEV)
        buf[::2] = r0.flatten().to(DEV)
        recon, target = buf[::2].view(r0.shape) if r0.dim() == 1 else buf.view(*r0.shape, 2)[..., 0], t0.to(DEV)
        assert not recon.is_contiguous()
    else:
        recon, target = r0.to(DEV), t0.to(DEV)
    recon.requires_grad_(True)
    target.requires_grad_(True)
    with variant_ctx(variant):
        _, thr, gt, eq = _selection(recon, target, k)
        loss = V._WorstK.apply(recon, target, k)
        (G.WK_COT * loss).backward()
    want = R.worst_k_loss(sel)
    print(f"{name} {variant}: n {sel['key'].size} k {k} threshold {thr:#010x} (restatement {int(sel['thr']):#010x}) count_gt {gt} "
          f"({sel['count_gt']}) count_eq {eq} ({sel['count_eq']}); loss {loss.item():.8g} ref64 {want:.8g}")
    assert (thr, gt, eq) == (int(sel["thr"]), sel["count_gt"], sel["count_eq"])
    assert close(loss.item(), want, LOSS_TOL)
    g = recon.grad.cpu().double().numpy().ravel()
    g64 = R.worst_k_grad(sel, G.WK_COT)
    fin = np.isfinite(g64)
    assert np.array_equal(np.isnan(g), np.isnan(g64)) and np.array_equal(g[~fin & ~np.isnan(g64)], g64[~fin & ~np.isnan(g64)])
    assert np.array_equal(g[fin] != 0, g64[fin] != 0) and np.all(np.abs(g[fin] - g64[fin]) <= WK_GRAD_TOL * np.abs(g64[fin]))
    assert torch.equal(target.grad.nan_to_num(7.0), -recon.grad.nan_to_num(-7.0))
    if name == "ties":
        assert eq > k - gt > 0
        tied = (sel["key"] == sel["thr"]) & (sel["d"] != 0)
        w = g[tied] / (G.WK_COT * 2.0 * sel["d"].astype(np.float64)[tied] / k)
        implied = G.WK_COT * 2.0 / k * float((R.worst_k_weights(sel) * sel["d"].astype(np.float64)).sum())
        print(f"ties {variant}: tie weight {w.min():.8f} .. {w.max():.8f} (exact {(k - gt) / eq:.8f}); gradient sum {g.sum():.8g} implied {implied:.8g}")
        assert np.all(np.abs(w - (k - gt) / eq) <= WK_GRAD_TOL * (k - gt) / eq)
        assert abs(g.sum() - implied) <= WK_GRAD_TOL * np.abs(g).sum()
    if name == "equal":
        assert loss.item() == 0.0 and not recon.grad.any() and not target.grad.any()
    if name == "nan":
        assert torch.isnan(loss)


@pytest.mark.selfcheck
@pytest.mark.parametrize("variant", ("contiguous", "wrap_channels_last"))
def test_two_runs_give_the_same_bits(variant):
    from autoregressive_diffusion_amd import vae_losses as V

    def run():
        out = []
        with variant_ctx(variant):
            m, lv, tg = operands("mid", variant)
            trio = V.recon_losses(m, lv, tg)
            sum(c * v for c, v in zip(G.COTS, trio)).backward()
            out += [*trio, m.grad, lv.grad, tg.grad]
            for fn in (V.l1_loss, V.mse_loss):
                m, lv, tg = operands("mid", variant)
                loss = fn(m, tg)
                loss.backward()
                out += [loss, m.grad, tg.grad]
            m, lv, tg = operands("mid", variant)
            loss = V.GaussianLoss(m, lv, tg)
            loss.backward()
            out += [loss, m.grad, lv.grad, tg.grad]
            for src, percent in (("mid", 0.2), ("ties", None)):
                if src == "mid":
                    r, _, t = operands("mid", variant)
                    loss = V.worst_k_percent_loss(r, t, percent=percent)
                else:
                    r0, t0, k = G.crafted("ties")
                    r, t = r0.to(DEV).requires_grad_(True), (channels_last(t0.to(DEV)) if variant.endswith("channels_last") else t0.to(DEV)).requires_grad_(True)
                    loss = V._WorstK.apply(r, t, k)
                loss.backward()
                out += [loss, r.grad, t.grad]
        return [o.detach().clone() for o in out]
    a, b = run(), run()
    assert len(a) == len(b) == 22 and all(torch.equal(x, y) for x, y in zip(a, b))


def test_only_requested_gradients_and_sign_of_zero():
    from autoregressive_diffusion_amd import vae_losses as V
    m, lv, tg = operands("tail", "channels_last", grad=False)
    _, _, want = fused64("tail")
    lv.requires_grad_(True)                                   # d logvar alone
    sum(c * v for c, v in zip(G.COTS, V.recon_losses(m, lv, tg))).backward()
    assert m.grad is None and tg.grad is None and rel(lv.grad.cpu(), want[1]) <= FUSED_GRAD_TOL
    lv.requires_grad_(False)
    lv.grad = None
    tg.requires_grad_(True)                                   # d target alone
    sum(c * v for c, v in zip(G.COTS, V.recon_losses(m, lv, tg))).backward()
    assert m.grad is None and lv.grad is None and rel(tg.grad.cpu(), want[2]) <= FUSED_GRAD_TOL
    assert tg.grad.stride() == tg.stride()
    lv.requires_grad_(True)                                   # a loss that does not use logvar leaves it without a gradient
    tg.grad = None
    V.recon_losses(m, lv, tg)[1].backward()
    assert lv.grad is None and tg.grad is not None
    r, t = m.clone().requires_grad_(True), tg.detach()
    V.worst_k_percent_loss(r, t, percent=0.5).backward()
    assert t.grad is None and int((r.grad != 0).sum()) == 48
    m2 = m.clone()
    m2.view(-1)[:7] = tg.detach().contiguous().view(-1)[:7]   # sign(0) = 0, as torch's L1
    m2.requires_grad_(True)
    V.l1_loss(m2, tg.detach()).backward()
    assert not m2.grad.view(-1)[:7].any() and torch.all(m2.grad.view(-1)[7:].abs() == m2.grad.view(-1)[7].abs())
    want = torch.sign(m2.detach() - tg.detach()) / m2.numel()
    assert rel(m2.grad, want) <= FUSED_GRAD_TOL


def test_nothing_synchronises_with_the_host():
    from autoregressive_diffusion_amd import vae_losses as V
    cots = [torch.tensor(c, device=DEV) for c in G.COTS]
    ops = [operands("tail", variant) for variant in ("contiguous", "channels_last")]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for m, lv, tg in ops:
            trio = V.recon_losses(m, lv, tg)
            (trio[0] * cots[0] + trio[1] * cots[1] + trio[2] * cots[2]).backward()
            (V.GaussianLoss(m, lv, tg) * cots[0]).backward()
            (V.l1_loss(m, tg) * cots[1]).backward()
            (V.mse_loss(m, tg) * cots[2]).backward()
            (V.worst_k_percent_loss(m, tg, percent=0.2) * cots[0]).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(m.grad).all()


def test_offsets_and_counts_beyond_32_bits():
    """An operand whose element offsets pass 2^31 (a view with a stride of 2^30 + 4 elements; 12.9 GB of address space, 20 elements
    touched) and a launch over more than 2^31 elements (broadcast views of 1030 values: nothing of that size is allocated)."""
    from autoregressive_diffusion_amd import vae_losses as V
    g = torch.Generator().manual_seed(2120)
    m0, lv0, tg0 = 0.6 * torch.randn(4, 5, generator=g), 0.7 * torch.randn(4, 5, generator=g) - 1, torch.rand(4, 5, generator=g) * 2 - 1
    step = 2 ** 30 + 4
    base = torch.empty(3 * step + 5, device=DEV)
    m = base.as_strided((4, 5), (step, 1))
    m.copy_(m0)
    m.requires_grad_(True)
    lv, tg = lv0.to(DEV).requires_grad_(True), tg0.to(DEV).requires_grad_(True)
    trio = V.recon_losses(m, lv, tg)
    sum(c * v for c, v in zip(G.COTS, trio)).backward()
    want_losses, termabs, want_grads = R.fused(m0, lv0, tg0, G.COTS)
    for name, got, want, ta in zip(LOSSES, trio, want_losses, termabs):
        print(f"offsets > 2^31: {name} {got.item():.8f} ref64 {want:.8f}")
        assert abs(got.item() - want) <= LOSS_TOL * ta
    for got, want in zip((m.grad, lv.grad, tg.grad), want_grads):
        assert rel(got.cpu(), want) <= FUSED_GRAD_TOL
    r = m.detach().requires_grad_(True)
    loss = V.worst_k_percent_loss(r, tg.detach(), percent=20.0)
    loss.backward()
    sel = R.select(m0, tg0, 4)
    assert close(loss.item(), R.worst_k_loss(sel), LOSS_TOL) and int((r.grad != 0).sum()) == 4
    del base, m, r
    rows = 2 ** 21 + 3                                        # 1030 (2^21 + 3) = 2 160 070 770 elements > 2^31
    a, b, c = (t.to(DEV) for t in (0.6 * torch.randn(1030, generator=g), 0.7 * torch.randn(1030, generator=g) - 1, torch.rand(1030, generator=g) * 2 - 1))
    big = [t.view(1, 1, 1, 1, 1030).expand(rows, 1, 1, 1, 1030) for t in (a, b, c)]
    assert big[0].numel() > 2 ** 31
    trio = V.recon_losses(*big)
    want_losses, termabs, _ = R.fused(a.cpu(), b.cpu(), c.cpu(), G.COTS)
    for name, got, want, ta in zip(LOSSES, trio, want_losses, termabs):
        print(f"{big[0].numel()} elements: {name} {got.item():.8f} ref64 {want:.8f} |diff| / mean|term| {abs(got.item() - want) / ta:.2e}")
        assert abs(got.item() - want) <= LOSS_TOL * ta


def test_one_vae_training_step_with_the_native_losses():
    """VAE([3, 32, 64, 8], 1 ResBlock) on (2, 3, 8, 8, 12), the smallest shape of tests/test_vae_train_gpu.py: loss = GaussianLoss +
    l1 on the same VAE.forward, once with the native losses and once with the torch formulas; the parameter gradients of the two
    runs within rel L2 5e-5 of each other (the project's bound for VAE gradients)."""
    from autoregressive_diffusion_amd import vae_losses as V
    from autoregressive_diffusion_amd.vae import VAE
    from test_vae_train_gpu import seed_params
    vae = seed_params(VAE(channels=[3, 32, 64, 8], n_res_blocks=1), 1611).to(DEV).train()
    g = torch.Generator().manual_seed(1612)
    x = torch.rand(2, 3, 8, 8, 12, generator=g) * 2 - 1
    ts, noise = (torch.rand(2, generator=g) * 0.1).to(DEV), torch.randn(2, 8, 2, 2, 3, generator=g).to(DEV)
    frames = channels_last(x.to(DEV))
    grads, losses = [], []
    for native in (True, False):
        vae.zero_grad(set_to_none=True)
        r_mean, r_logvar, _, _ = vae(x.to(DEV), t_sample=ts, noise=noise)
        if native:
            loss = V.GaussianLoss(r_mean, r_logvar, frames) + V.l1_loss(r_mean, frames)
        else:
            loss = R.gaussian(r_mean, r_logvar, frames) + torch.nn.functional.l1_loss(r_mean, frames)
        loss.backward()
        losses.append(loss.item())
        grads.append({n: p.grad.clone() for n, p in vae.named_parameters()})
    errs = {n: rel(grads[0][n].cpu(), grads[1][n].cpu()) for n in grads[0]}
    print(f"loss native {losses[0]:.8f} torch {losses[1]:.8f}")
    for n in sorted(errs, key=errs.get, reverse=True)[:8]:
        print(f"grad {n}: rel L2 native vs torch losses {errs[n]:.2e}")
    assert abs(losses[0] - losses[1]) <= LOSS_TOL * abs(losses[1])
    assert set(grads[0]) == set(grads[1]) and max(errs.values()) <= 5e-5
