"""What the element-by-element GPU tests (test_glue_stages_gpu.py, test_step_edge_gpu.py, test_weight_stages_gpu.py) share  --
TEST INFRASTRUCTURE: NaN-prefilled output buffers and the ways a kernel's output is held to a float64 restatement (bf16 outputs,
fp32 reductions, fp32 elementwise results, exact results).  The bounds themselves (bound_bf16, bound_f32, U_F32_64) live in
glue_oracle.py.  Every figure is printed as `<tag> <case> <tensor> <worst error / bound>` (tags: GLUE, EDGE, WEIGHT)."""
import torch

import glue_oracle as GO

DEV = "cuda"
BF16 = torch.bfloat16
NAN = float("nan")


def out(*shape, dtype=BF16, fill=NAN):
    """An output buffer the kernel must write completely: pre-filled with NaN (accumulators: zeros)."""
    return torch.full(shape, fill, dtype=dtype, device=DEV)


def ratio(case, name, got, ref, bound, tag="GLUE"):
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{case} {name}: non-finite values (an element the kernel never wrote?)"
    err = (got - ref).abs()
    live = bound > 0
    dead_ok = bool((err[~live] == 0).all())
    worst = (err[live] / bound[live]).max().item() if bool(live.any()) else 0.0
    print(f"{tag} {case} {name} {worst:.3f}")
    assert dead_ok, f"{case} {name}: an element whose reference is exactly 0 came back non-zero"
    assert worst <= 1.0, f"{case} {name}: worst |got - ref| / bound = {worst:.3f} over {err.numel()} elements"


def hold_bf16(case, name, got, pair, tag="GLUE"):
    """bf16 output: 2^-8 |ref| + 2^-18 mag."""
    ratio(case, name, got, pair[0], GO.bound_bf16(*pair), tag)


def hold_f32(case, name, got, pair, tag="GLUE"):
    """fp32 reduction: 2^-17 mag."""
    ratio(case, name, got, pair[0], GO.bound_f32(pair[1]), tag)


def hold_f32_elem(case, name, got, pair, tag="GLUE"):
    """fp32 elementwise output: 2^-18 mag."""
    ratio(case, name, got, pair[0], GO.U_F32_64 * pair[1], tag)


def hold_exact(case, name, got, ref, tag="GLUE"):
    got = got.detach().cpu()
    ref = ref.reshape(got.shape)
    assert bool(torch.isfinite(got.float()).all()), f"{case} {name}: non-finite values"
    assert bool((got.double() == ref.double()).all()), f"{case} {name}: {int((got.double() != ref.double()).sum())} elements differ (exact probe)"
    print(f"{tag} {case} {name} exact")
