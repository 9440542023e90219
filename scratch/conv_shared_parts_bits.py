"""Bit identity of the forward / dgrad conv kernels between two trees (profiles/conv_shared_parts.txt, step 2).

  python scratch/conv_shared_parts_bits.py run DIR        in a tree, in a fresh process: every case below on seeded inputs; every output
                                                          and gradient tensor goes to DIR/tensors.pt, the kernel instantiations each
                                                          case launched (ops.census_start / census_stop) to DIR/census.json
  python scratch/conv_shared_parts_bits.py compare A B    torch.equal on every tensor of the two runs, no tolerance; the union of the
                                                          instantiations; --delete removes the two tensor files afterwards

Cases: the smallest shapes at which the test suite reaches each kernel family, each with the three epilogues (none, emb-scale + SiLU,
mp_sum with residual -- once with a residual that reaches the +-256 clip, once with the clip armed but not reached), forward and backward.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

DEV, BF16 = "cuda", torch.bfloat16
EPIS = ("none", "emb_silu", "mpsum_clipped", "mpsum_armed")


def bf(x):
    return x.to(DEV, BF16).contiguous()


def weight(*shape):
    fan = 1
    for d in shape[1:]:
        fan *= d
    return torch.nn.Parameter((torch.randn(*shape) / fan ** 0.5).to(DEV))


def conv3x3_case(ops, out, name, gated, B, T, H, W, cin, cout):
    """gated: DART training layout (B sequences x 2 slots x T frames); plain: N = B * T frames."""
    N = B * 2 * T if gated else B * T
    for epi in EPIS:
        torch.manual_seed(11)
        p2, p3 = weight(cout, cin, 3, 3), weight(cout, cin, 2, 3, 3)
        bank = ops.WeightBank()
        pw2, pw3 = bank.add(p2), (bank.add(p3) if gated else None)
        bank.prepare(training=True)
        x = bf(torch.randn(N, H, W, cin)).requires_grad_(True)
        gate = (torch.rand(N) * 0.5 + 0.05).to(DEV).requires_grad_(True)
        cs = (1 + 0.3 * torch.randn(N, cout)).to(DEV).requires_grad_(True)
        res = bf(torch.randn(N, H, W, cout) * (200 if epi == "mpsum_clipped" else 2)).requires_grad_(True)
        gy = bf(torch.randn(N, H, W, cout))
        kw = {} if epi == "none" else dict(cscale=cs) if epi == "emb_silu" else dict(res=res, ta=0.9, tb=0.4, clip=256.0, grad_private=True)
        y = ops.gated_conv_train(x, gate, pw2, pw3, B, T, **kw) if gated else ops.conv(x, pw2, **kw)
        if epi.startswith("mpsum"):
            frac = float((y.detach().abs() >= 256).float().mean())
            assert (frac > 0.01) == (epi == "mpsum_clipped"), (name, epi, frac)
        y.backward(gy)
        bank.backward()
        torch.cuda.synchronize()
        t = dict(y=y, dx=x.grad, dw2=p2.grad, gy_after=gy)
        if gated:
            t.update(dw3=p3.grad, dgate=gate.grad)
        if epi == "emb_silu":
            t["dcscale"] = cs.grad
        if epi.startswith("mpsum"):
            t["dres"] = res.grad
        for k, v in t.items():
            assert v is not None, (name, epi, k)
            out[f"{name}/{epi}/{k}"] = v.detach().cpu().clone()


def conv1x1_mpsum_case(ops, out, name, N, H, cin, cout, clip):
    torch.manual_seed(cin + N)
    p = weight(cout, cin, 1, 1)
    bank = ops.WeightBank()
    pw = bank.add(p)
    bank.prepare(training=True)
    x = bf(torch.randn(N, H, H, cin)).requires_grad_(True)
    res = bf(torch.randn(N, H, H, cout) * 1.5).requires_grad_(True)
    y = ops.conv(x, pw, res=res, ta=0.8, tb=0.6, clip=clip)
    y.backward(bf(torch.randn(N, H, H, cout)))
    bank.backward()
    torch.cuda.synchronize()
    for k, v in dict(y=y, dx=x.grad, dres=res.grad, dw=p.grad).items():
        out[f"{name}/{k}"] = v.detach().cpu().clone()


def act_bwd_case(ops, _lib, out, name, H, C1, C2, Cout, N):
    """The decoder skip conv's dgrad with the mp_cat + mp_silu adjoint as its epilogue (conv1x1_glds_kernel<true> from 8192 positions on)."""
    torch.manual_seed(H + C1 + C2)
    C = C1 + C2
    p = weight(Cout, C, 1, 1)
    bank = ops.WeightBank()
    pw = bank.add(p)
    bank.prepare(training=True)
    g, da, xo = bf(torch.randn(N, H, H, Cout)), bf(torch.randn(N, H, H, C)), bf(torch.randn(N, H, H, C) * 1.5)
    dx = torch.zeros(N, H, H, C1, dtype=BF16, device=DEV)
    dskip = torch.zeros(N, H, H, C2, dtype=BF16, device=DEV)
    ops._conv_launch(g, None, pw.wb, None, dx, None, None, 1, 1, N, H, H, Cout, pw.CinPb, C, pw.CoutPb, 1,
                     epi=_lib.EPI_ACT_BWD, act_bwd=(da, xo, dskip, None, C1, 0.9, 1.2, 1.0))
    torch.cuda.synchronize()
    out[f"{name}/dx"], out[f"{name}/dskip"] = dx.cpu(), dskip.cpu()


def eval_one_frame_case(ops, out, name, B, H, cin, cout, epi):
    """tests/test_ops_gpu.py: test_gated_conv_eval_one_frame_splitk (conv_eval1_kernel; ops.SPLITK = 0: the split-K pair with its reduce launch)."""
    torch.manual_seed(cin + H)
    p2, p3 = torch.nn.Parameter(torch.randn(cout, cin, 3, 3).to(DEV)), torch.nn.Parameter(torch.randn(cout, cin, 2, 3, 3).to(DEV))
    bank = ops.WeightBank()
    pw2, pw3 = bank.add(p2), bank.add(p3)
    bank.prepare(training=False)
    x, pad = bf(torch.randn(B, H, H, cin)), bf(torch.randn(B, 2, H, H, cin))
    g = (torch.rand(B) * 0.6 + 0.05).to(DEV)
    kw = {}
    if epi == "silu":
        kw = dict(cscale=(torch.rand(B, cout) + 0.5).to(DEV))
    elif epi == "mpsum":
        kw = dict(res=bf(torch.randn(B, H, H, cout)), ta=0.7, tb=0.5, clip=2.0)
    keep = ops.SPLITK
    try:
        for sk in (1, 0):
            ops.SPLITK = sk
            with torch.no_grad():
                out[f"{name}/splitk{sk}"] = ops.gated_conv_eval(x, g, pw2, pw3, B, 1, pad, ctx_T=2, **kw).cpu()
    finally:
        ops.SPLITK = keep


def few_tiles_case(ops, out, name, N, H, C1, C2, cout):
    """tests/test_ops_gpu.py: test_conv1x1_few_tiles_same_bits_on_both_tile_widths (conv1x1_few_kernel and the register-staged few-tile forms)."""
    torch.manual_seed(N + H + C1)
    p = weight(cout, C1 + C2, 1, 1)
    bank = ops.WeightBank()
    pw = bank.add(p)
    bank.prepare(training=False)
    x, skip = bf(torch.randn(N, H, H, C1) * 1.5), bf(torch.randn(N, H, H, C2))
    xc = torch.cat([x, skip], -1).contiguous()
    res = bf(torch.randn(N, H, H, cout))
    keep = ops.BIG_TILE
    try:
        for bits in (512, 64, 0):
            ops.BIG_TILE = (keep & ~(64 | 512)) | bits
            with torch.no_grad():
                y, a = ops.conv_cat_act(x, skip, 0.83, 1.21, pw)
                t = dict(y=y, act=a, plain=ops.conv(xc, pw), mpsum=ops.conv(xc, pw, res=res, ta=0.8, tb=0.6, clip=2.0))
            for k, v in t.items():
                out[f"{name}/bits{bits}/{k}"] = v.cpu()
    finally:
        ops.BIG_TILE = keep


def run(outdir):
    from autoregressive_diffusion_amd import ops, _lib
    os.makedirs(outdir, exist_ok=True)
    out, census = {}, {}
    cases = []
    # gated (B, T, H, W, cin, cout): register-staged | conv_glds PW = 16, NT = 2 (dgrad: NT = 1) | conv_stream, ALIAS true (forward) and
    # false (dgrad) | conv_glds PW = 8 | conv_glds resident layout (32 -> 96) | non-square
    for B, T, H, W, cin, cout in [(1, 4, 8, 8, 32, 64), (1, 4, 16, 16, 32, 64), (1, 4, 16, 16, 32, 32), (1, 4, 8, 8, 128, 128),
                                  (1, 4, 16, 16, 32, 96), (1, 4, 16, 32, 32, 32)]:
        n = f"gated_B{B}_T{T}_{H}x{W}_{cin}to{cout}"
        cases.append((n, lambda n=n, a=(B, T, H, W, cin, cout): conv3x3_case(ops, out, n, True, *a)))
    # plain (N, H, cin, cout): conv_glds without context phases, NT = 2 (dgrad: NT = 1) | conv_plain_stream | ... with a ragged Cout |
    # conv_glds PW = 8 without context phases
    for N, H, cin, cout in [(6, 16, 32, 64), (8, 128, 32, 32), (8, 128, 32, 24), (4, 8, 64, 64)]:
        n = f"plain_N{N}_{H}x{H}_{cin}to{cout}"
        cases.append((n, lambda n=n, a=(1, N, H, H, cin, cout): conv3x3_case(ops, out, n, False, *a)))
    for N, H, cin, cout, clip in [(9, 32, 128, 128, 2.0), (15, 24, 64, 200, 0.0)]:
        n = f"conv1x1_mpsum_N{N}_{H}_{cin}to{cout}_clip{clip}"
        cases.append((n, lambda n=n, a=(N, H, cin, cout, clip): conv1x1_mpsum_case(ops, out, n, *a)))
    cases.append(("act_bwd_32_64+64to64_N8", lambda: act_bwd_case(ops, _lib, out, "act_bwd_32_64+64to64_N8", 32, 64, 64, 64, 8)))
    for B, H, cin, cout, epi in [(1, 8, 256, 256, "silu"), (1, 16, 128, 128, "mpsum"), (2, 32, 64, 64, "none"), (1, 8, 96, 160, "mpsum"),
                                 (1, 64, 32, 32, "silu"), (3, 4, 128, 64, "none"), (4, 64, 32, 32, "mpsum"), (3, 32, 64, 96, "silu")]:
        n = f"eval1_B{B}_{H}_{cin}to{cout}_{epi}"
        cases.append((n, lambda n=n, a=(B, H, cin, cout, epi): eval_one_frame_case(ops, out, n, *a)))
    for N, H, C1, C2, cout in [(1, 8, 256, 256, 256), (1, 16, 256, 128, 128), (1, 32, 64, 32, 64), (8, 8, 256, 256, 256), (1, 64, 64, 32, 32)]:
        n = f"few_N{N}_{H}_{C1}+{C2}to{cout}"
        cases.append((n, lambda n=n, a=(N, H, C1, C2, cout): few_tiles_case(ops, out, n, *a)))
    for name, fn in cases:
        ops.census_start()
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            census[name] = ops.census_stop()
        print(name, "->", ", ".join(sorted(k for k in census[name] if "conv" in k)), flush=True)
    torch.save(out, os.path.join(outdir, "tensors.pt"))
    with open(os.path.join(outdir, "census.json"), "w") as f:
        json.dump(census, f, indent=1, sort_keys=True)
    print(f"saved {len(out)} tensors, {sum(v.numel() for v in out.values())} elements")


def compare(da, db, delete):
    a, b = torch.load(os.path.join(da, "tensors.pt")), torch.load(os.path.join(db, "tensors.pt"))
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    differ, nonfinite, zero, groups = [], 0, [], {}
    for k in sorted(a):
        same = a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k])
        if not same:
            differ.append(k)
        nonfinite += int((~a[k].float().isfinite()).sum())
        g = k.split("/")[0]
        groups[g] = groups.get(g, 0) + 1
        if a[k].numel() == 0 or not a[k].float().abs().max() > 0:
            zero.append(k)
    for g in sorted(groups):
        print(f"{g}: {groups[g]} tensors")
    print(f"compared {len(a)} tensors, {sum(v.numel() for v in a.values())} elements: {len(differ)} differ {differ[:10]}; non-finite: {nonfinite}; all-zero tensors: {zero}")
    ca, cb = json.load(open(os.path.join(da, "census.json"))), json.load(open(os.path.join(db, "census.json")))
    print("the two runs launched the same instantiations per case:", ca == cb)
    union = sorted({k for v in ca.values() for k in v if "conv" in k and "wgrad" not in k})
    print("forward / dgrad conv instantiations launched (union over the cases):")
    for k in union:
        print("  ", k)
    if delete:
        os.remove(os.path.join(da, "tensors.pt"))
        os.remove(os.path.join(db, "tensors.pt"))
    return 0 if not differ and ca == cb else 1


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3], "--delete" in sys.argv))
