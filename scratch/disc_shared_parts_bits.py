"""Bit identity of the discriminator kernels between two trees (profiles/disc_shared_parts.txt, step 2).

  python scratch/disc_shared_parts_bits.py run DIR        in a tree, in a fresh process: every case below on seeded inputs; every output
                                                          and gradient tensor goes to DIR/tensors.pt
  python scratch/disc_shared_parts_bits.py compare A B    torch.equal on every tensor of the two runs, no tolerance; one line per case

Cases: the shapes of the stage tests (tests/test_discriminator_gpu.py, tests/test_discriminator3d_gpu.py: ragged tiles, both NB, the
scalar and the vector staging paths, 1 and 9 taps, planes skipped at the T border, the stride-2 stem), the two norm backward passes
and the whole nets.  Per stage case: the forward with and without prologue and with the residual, the statistics partials and the
finalized stats, the data gradient, and the weight and bias gradients with default slabs and with _MAX_SLABS = 2.
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

DEV = "cuda"
CONV2 = [(3, 7, 5, 3, 32, 9), (2, 24, 40, 32, 32, 9), (1, 16, 16, 96, 64, 9), (2, 8, 8, 64, 2, 9), (3, 6, 10, 32, 64, 1)]
CONV3 = [(2, 1, 7, 5, 32, 32, 27), (1, 3, 18, 20, 32, 64, 27), (2, 4, 9, 11, 96, 32, 27), (2, 2, 8, 8, 64, 2, 27), (2, 3, 6, 10, 32, 64, 1)]
STEMS = [(2, 1, 7, 5, 3, 32), (2, 5, 18, 22, 6, 32), (3, 2, 33, 17, 8, 64), (1, 4, 4, 4, 1, 32)]
BN_BWD = [(3, 7, 5, 32), (2, 24, 40, 64)]
GN_BWD = [(2, 1, 7, 5, 32), (2, 3, 9, 11, 64), (1, 2, 6, 6, 96)]


def ident(s):
    return "x".join(map(str, s))


def rnd(g, *shape):
    return torch.randn(*shape, generator=g).to(DEV)


def pro_vectors(g, *shape):
    """s in 0.5 .. 1.5, |t| in 2 .. 3 with random sign: a halo filled with lrelu(t) instead of 0 would show."""
    s = 0.5 + torch.rand(*shape, generator=g)
    t = (2.0 + torch.rand(*shape, generator=g)) * torch.where(torch.rand(*shape, generator=g) > 0.5, 1.0, -1.0)
    return s.to(DEV), t.to(DEV)


def with_slabs(d, fn, keep):
    """fn() with the default slab budget and with _MAX_SLABS = 2 (the work items wrap)."""
    keep["dw"], keep["db"] = fn()
    old = d._MAX_SLABS
    try:
        d._MAX_SLABS = 2
        keep["dw_2slabs"], keep["db_2slabs"] = fn()
    finally:
        d._MAX_SLABS = old


def stage2(d, shape):
    N, H, W, Cin, Cout, taps = shape
    g = torch.Generator().manual_seed(100 + Cin + Cout)
    k = 3 if taps == 9 else 1
    x, w, b = rnd(g, N, H, W, Cin), rnd(g, Cout, Cin, k, k) / math.sqrt(taps * Cin), 0.3 * rnd(g, Cout)
    pro = pro_vectors(g, Cin)
    res, dy = rnd(g, N, H, W, Cout), rnd(g, N, H, W, Cout)
    wp, t = d.pack_weight(w), {}
    stats = Cout % 32 == 0
    t["y"], part = d.conv(x, wp, b, Cout, taps, stats=stats)
    t["y_pro"], part_pro = d.conv(x, wp, b, Cout, taps, pro=pro, stats=stats)
    t["y_pro_res"] = d.conv(x, wp, b, Cout, taps, pro=pro, res=res, res_scale=d._SCALE)[0]
    if stats:
        gamma, beta = 1 + 0.3 * rnd(g, Cout), 0.3 * rnd(g, Cout)
        rm, rv = 0.2 * rnd(g, Cout), (0.5 + torch.rand(Cout, generator=g)).to(DEV)
        t["part"], t["part_pro"] = part, part_pro
        t["stats"] = d.finalize(part_pro, gamma, beta, rm, rv, 0.1, 1e-5)
        t["running_mean"], t["running_var"] = rm, rv
    t["dx"] = d.conv(dy, d.pack_weight_dgrad(w), None, Cin, taps)[0]
    with_slabs(d, lambda: d.wgrad(x, dy, taps, pro=pro), t)
    return t


def stage3(d, shape, stride):
    N, T, H, W, Cin, Cout = shape[:6]
    taps = shape[6] if stride == 1 else 27
    g = torch.Generator().manual_seed(300 + Cin + Cout + T)
    o = lambda n: (n - 1) // stride + 1
    k = 1 if taps == 1 else 3
    x, w, b = rnd(g, N, T, H, W, Cin), rnd(g, Cout, Cin, k, k, k) / math.sqrt(k ** 3 * Cin), 0.3 * rnd(g, Cout)
    pro = pro_vectors(g, N, Cin)
    res, dy = rnd(g, N, o(T), o(H), o(W), Cout), rnd(g, N, o(T), o(H), o(W), Cout)
    t = {}
    if taps == 1:                                        # the 1x1x1 shortcut: the 2-D kernels over the N T planes
        wp = d.pack_weight(w[..., 0])
        t["y"], t["part"] = d.conv(d._planes(x), wp, b, Cout, 1, stats=True)
        t["y_res"] = d.conv(d._planes(x), wp, b, Cout, 1, res=d._planes(res), res_scale=d._SCALE)[0]
        t["dx"] = d.conv(d._planes(dy), d.pack_weight_dgrad(w[..., 0]), None, Cin, 1)[0]
        with_slabs(d, lambda: d.wgrad(d._planes(x), d._planes(dy), 1), t)
        return t
    wp = d.pack_weight3(w)
    stats = Cout % 32 == 0
    t["y"], part = d.conv3(x, wp, b, Cout, stride=stride, stats=stats)
    if stride == 1:
        t["y_pro"], part = d.conv3(x, wp, b, Cout, pro=pro, stats=stats)
        t["y_pro_res"] = d.conv3(x, wp, b, Cout, pro=pro, res=res, res_scale=d._SCALE)[0]
        t["dx"] = d.conv3(dy, d.pack_weight3_dgrad(w), None, Cin)[0]
    else:
        t["dx"] = d.stem_dgrad3(dy, wp, T, H, W, Cin)
    if stats:
        t["part"] = part
        t["stats"] = d.gn_finalize(part, 1 + 0.3 * rnd(g, Cout), 0.3 * rnd(g, Cout))
    with_slabs(d, lambda: d.wgrad3(x, dy, stride, pro=pro if stride == 1 else None), t)
    return t


def bn_backward(d, shape):
    N, H, W, C = shape
    g = torch.Generator().manual_seed(13)
    z, da, add = 0.5 + 1.5 * rnd(g, N, H, W, C), rnd(g, N, H, W, C), rnd(g, N, H, W, C)
    gamma, beta = 1 + 0.3 * rnd(g, C), 0.3 * rnd(g, C)
    var, mean = torch.var_mean(z.reshape(-1, C), 0, unbiased=False)
    rstd = torch.rsqrt(var + 1e-5)
    stats = torch.stack((mean, var, gamma * rstd, beta - mean * gamma * rstd, rstd)).contiguous()
    t = {}
    for mode in (False, True):
        dx, sums = d.bn_bwd(da, z, stats, add, 0.5, eval_mode=mode)
        t[f"dx_eval{int(mode)}"], t[f"sums_eval{int(mode)}"] = dx, sums
    return t


def gn_backward(d, shape):
    N, T, H, W, C = shape
    g = torch.Generator().manual_seed(13)
    z, da, add = 0.5 + 1.5 * rnd(g, N, T, H, W, C), rnd(g, N, T, H, W, C), rnd(g, N, T, H, W, C)
    gamma, beta = 1 + 0.3 * rnd(g, C), 0.3 * rnd(g, C)
    zg = z.reshape(N, -1, 32, C // 32).permute(0, 2, 1, 3).reshape(N, 32, -1)
    var, mean = torch.var_mean(zg, 2, unbiased=False)
    mean, var = mean.repeat_interleave(C // 32, 1), var.repeat_interleave(C // 32, 1)
    rstd = torch.rsqrt(var + 1e-5)
    stats = torch.stack((mean, var, gamma * rstd, beta - mean * gamma * rstd, rstd)).contiguous()
    dx, sums = d.gn_bwd(da, z, stats, gamma, add, 0.5)
    return dict(dx=dx, sums=sums)


def whole(net, x, loss=None):
    """Forward plus every parameter and input gradient."""
    x = x.clone().requires_grad_(True)
    y = net(x) if loss is None else loss(x)
    (y.square().mean() if loss is None else y).backward()
    t = {"y": y}
    if x.grad is not None:                               # discriminator_loss detaches its inputs
        t["dx"] = x.grad
    for n, p in net.named_parameters():
        if p.grad is not None:                           # Discriminator2D.conv_norm_out is unused, as in the reference
            t["grad/" + n] = p.grad
    assert any(k.startswith("grad/") for k in t)
    for n, b in net.named_buffers():
        t["buffer/" + n] = b
    return t


def nets(d):
    out = {}
    for mode in ("train", "eval"):
        torch.manual_seed(1811)
        net = d.Discriminator2D(3, (64, 64, 64)).to(DEV)
        getattr(net, mode)()
        out[f"net2d_{mode}"] = lambda net=net: whole(net, torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(DEV))
    torch.manual_seed(1812)
    n3 = d.Discriminator3D(3, (64, 64)).to(DEV).train()
    out["net3d"] = lambda: whole(n3, torch.randn(2, 3, 4, 20, 24, generator=torch.Generator().manual_seed(6)).to(DEV))
    g = torch.Generator().manual_seed(7)
    # 1 + 2 channels, one clip: the critic sees (2, 3, 4, 32, 32), as in tests/golden/make_golden_disc.py
    frames, recon = torch.randn(1, 1, 4, 32, 32, generator=g).to(DEV), torch.randn(1, 2, 4, 32, 32, generator=g).to(DEV)
    for which in ("discriminator_loss", "vae_loss"):
        torch.manual_seed(1813)
        mixed = d.MixedDiscriminator(3).to(DEV).train()
        out[f"mixed_{which}"] = lambda mixed=mixed, which=which: whole(mixed, recon, lambda r: getattr(mixed, which)(frames, r))
    return out


def run(outdir):
    from autoregressive_diffusion_amd import discriminator as d
    os.makedirs(outdir, exist_ok=True)
    cases = {}
    for s in CONV2:
        cases["conv2d_" + ident(s)] = lambda s=s: stage2(d, s)
    for s in CONV3:
        cases["conv3d_" + ident(s)] = lambda s=s: stage3(d, s, 1)
    for s in STEMS:
        cases["stem_" + ident(s)] = lambda s=s: stage3(d, s, 2)
    for s in BN_BWD:
        cases["bn_bwd_" + ident(s)] = lambda s=s: bn_backward(d, s)
    for s in GN_BWD:
        cases["gn_bwd_" + ident(s)] = lambda s=s: gn_backward(d, s)
    cases.update(nets(d))
    out = {}
    for name, fn in cases.items():
        t = fn()
        torch.cuda.synchronize()
        for k, v in t.items():
            assert v is not None, (name, k)
            out[f"{name}//{k}"] = v.detach().cpu().clone()
        print(name, len(t), "tensors", flush=True)
    torch.save(out, os.path.join(outdir, "tensors.pt"))
    print(f"saved {len(out)} tensors, {sum(v.numel() for v in out.values())} elements")


def compare(da, db):
    a, b = torch.load(os.path.join(da, "tensors.pt")), torch.load(os.path.join(db, "tensors.pt"))
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    differ, nonfinite, zero, groups = [], 0, [], {}
    for k in sorted(a):
        if not (a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k])):
            differ.append(k)
        nonfinite += int((~a[k].float().isfinite()).sum())
        g = k.split("//")[0]
        groups[g] = groups.get(g, 0) + 1
        if a[k].numel() == 0 or not a[k].float().abs().max() > 0:
            zero.append(k)
    for g in sorted(groups):
        print(f"{g}: {groups[g]} tensors, {sum(k.split('//')[0] == g for k in differ)} differ")
    print(f"compared {len(a)} tensors, {sum(v.numel() for v in a.values())} elements: {len(differ)} differ {differ[:10]}; "
          f"non-finite: {nonfinite}; all-zero tensors: {zero}")
    return 0 if not differ else 1


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
