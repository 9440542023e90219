"""Bit identity of the bf16 weight-gradient kernels between two trees (profiles/wgrad_shared_parts.txt, step 2).

  python scratch/wgrad_shared_parts_bits.py run DIR        in a tree, in a fresh process: every case below on seeded inputs; every weight
                                                           gradient goes to DIR/tensors.pt, the kernel instantiations each case launched
                                                           to DIR/census.json
  python scratch/wgrad_shared_parts_bits.py compare A B    torch.equal on every tensor of the two runs, no tolerance; the union of the
                                                           weight-gradient instantiations must hold all 17 of conv_wgrad.hip

Helpers and the gated layout are those of conv_shared_parts_bits.py; the gate coefficients are not powers of two, so the bf16 rounding
of the coefficient folded into dy takes part in every gated result.
"""
import json
import os
import sys

import torch

from conv_shared_parts_bits import DEV, bf, weight

EXPECTED = ([f"conv_wgrad_kernel<9,{pw},{t},{t}>" for pw in (16, 8, 4, 2) for t in (2, 1)] + [f"conv_wgrad_kernel<1,16,{t},{t}>" for t in (2, 1)]
            + [f"conv_wgrad_glds_kernel<{t},{t},1,{pw}>" for pw in (16, 8) for t in (2, 1)]
            + ["conv_wgrad_stream_kernel<4>", "conv_wgrad_stream_kernel<8>", "wgrad1x1_glds_kernel<2>"])


def conv_case(ops, out, name, gated, B, T, H, W, cin, cout, k=3):
    """gated: DART training layout (B sequences x 2 slots x T frames), 3x3; plain: N = B * T frames, k x k."""
    N = B * 2 * T if gated else B * T
    torch.manual_seed(11)
    p2, p3 = weight(cout, cin, k, k), weight(cout, cin, 2, 3, 3)
    bank = ops.WeightBank()
    pw2, pw3 = bank.add(p2), (bank.add(p3) if gated else None)
    bank.prepare(training=True)
    x = bf(torch.randn(N, H, W, cin)).requires_grad_(True)
    gate = (torch.rand(N) * 0.5 + 0.05).to(DEV).requires_grad_(True)
    gy = bf(torch.randn(N, H, W, cout))
    y = ops.gated_conv_train(x, gate, pw2, pw3, B, T) if gated else ops.conv(x, pw2)
    y.backward(gy)
    bank.backward()
    torch.cuda.synchronize()
    out[f"{name}/dw2"] = p2.grad.detach().cpu().clone()
    if gated:
        out[f"{name}/dw3"] = p3.grad.detach().cpu().clone()


def run(outdir):
    from autoregressive_diffusion_amd import ops
    os.makedirs(outdir, exist_ok=True)
    out, census = {}, {}
    # (name, WGRAD_VARIANT, gated, B, T, H, W, cin, cout, k)
    lds_dma = [("gated_16x16_64to64", True, 1, 4, 16, 16, 64, 64), ("plain_N6_16x16_32to64", False, 1, 6, 16, 16, 32, 64),
               ("gated_8x8_128to128", True, 1, 4, 8, 8, 128, 128), ("gated_8x8_32to64", True, 1, 4, 8, 8, 32, 64)]
    cases = [("gated_B1_T4_16x16_32to32", 0, True, 1, 4, 16, 16, 32, 32, 3),            # streaming, 4x16-pixel tiles
             ("gated_B9_T2_64x64_32to32", 0, True, 9, 2, 64, 64, 32, 32, 3)]            # ... more 4x16 tiles than the weights own slabs: 8x16
    cases += [(n, 0, *c, 3) for n, *c in lds_dma]
    cases += [(n + "_regstaged", -1, *c, 3) for n, *c in lds_dma]
    cases += [(f"plain_N6_{h}x{h}_{c}to{c}", 0, False, 1, 6, h, h, c, c, 3) for h in (4, 2) for c in (64, 32)]
    cases += [("conv1x1_N9_32x32_128to128", 0, False, 1, 9, 32, 32, 128, 128, 1), ("conv1x1_N64_64x64_32to96", 0, False, 1, 64, 64, 64, 32, 96, 1),
              ("conv1x1_N9_32x32_64to64_regstaged", -1, False, 1, 9, 32, 32, 64, 64, 1),
              ("conv1x1_N130_1x1_64to96", 0, False, 1, 130, 1, 1, 64, 96, 1),           # ragged last position tile
              ("gated_16x16_96to160", 0, True, 1, 4, 16, 16, 96, 160, 3)]               # ragged channel blocks
    keep = ops.WGRAD_VARIANT
    for name, variant, *c in cases:
        ops.WGRAD_VARIANT = variant
        ops.census_start()
        try:
            conv_case(ops, out, name, *c)
            torch.cuda.synchronize()
        finally:
            census[name] = ops.census_stop()
            ops.WGRAD_VARIANT = keep
        print(name, "->", ", ".join(sorted(k for k in census[name] if "wgrad" in k)), flush=True)
    torch.save(out, os.path.join(outdir, "tensors.pt"))
    with open(os.path.join(outdir, "census.json"), "w") as f:
        json.dump(census, f, indent=1, sort_keys=True)
    print(f"saved {len(out)} tensors, {sum(v.numel() for v in out.values())} elements")


def compare(da, db):
    a, b = torch.load(os.path.join(da, "tensors.pt")), torch.load(os.path.join(db, "tensors.pt"))
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    differ = [k for k in sorted(a) if not (a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]))]
    nonfinite = sum(int((~a[k].float().isfinite()).sum()) for k in a)
    zero = [k for k in sorted(a) if a[k].numel() == 0 or not a[k].float().abs().max() > 0]
    print(f"compared {len(a)} tensors, {sum(v.numel() for v in a.values())} elements: {len(differ)} differ {differ[:10]}; non-finite: {nonfinite}; "
          f"all-zero tensors: {zero}")
    ca, cb = json.load(open(os.path.join(da, "census.json"))), json.load(open(os.path.join(db, "census.json")))
    print("the two runs launched the same instantiations per case:", ca == cb)
    union = sorted({k.split(" [")[0] for v in ca.values() for k in v if "wgrad" in k})
    print("weight-gradient instantiations launched (union over the cases):")
    for k in union:
        print("  ", k)
    missing = sorted(set(EXPECTED) - {k.replace(" ", "").replace("void", "") for k in union})
    print(f"of the {len(EXPECTED)} instantiations of conv_wgrad.hip, missing from the union: {missing}")
    return 0 if not differ and not zero and not nonfinite and ca == cb and not missing else 1


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
