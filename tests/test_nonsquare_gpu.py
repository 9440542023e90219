"""Non-square images (H != W) through every kernel that indexes rows and columns, against the CPU oracle.

Every 3x3 kernel takes H and W separately and picks its tile geometry from both; on a square image `ntx` and `nty`, `Ho` and `Wo`,
a row stride and a column stride are the same number, and whole dispatch branches (8x16 tiles with H % 16 != 0, several frames
per tile together with several tile rows, an odd number of 4-row tiles) cannot be reached.  This file runs the conv families
(forward, data gradient, weight gradient: against the fp32 oracle, in the bf16-faithful form of test_verification_gpu.py and with
the integer-exact weight gradient), the resampling / activation / DART passes, the attention modules, Blocks, whole training
steps and a cached rollout frame at H != W.  The test bodies are the ones of the square suites (test_ops_gpu.py,
test_verification_gpu.py: their `_..._case(H, W, ...)` helpers), so are the bounds.

A case that silently fell back to another kernel family would prove nothing: every conv case reads the dispatch census around
its launches (ops.census_peek: conftest.py owns start / stop) and asserts the family it was aimed at, and
test_python_mirrors_name_the_launched_family holds ops._s2ctx_family and the KernelProfile keys of ops._conv_launch /
_wgrad_launch_group -- hand-written Python mirrors of the C dispatch -- against what the library launched.

New here, for the bf16-faithful forward / data-gradient comparisons with a linear epilogue (none, mp_sum): per element
|got - ref| <= 2^-7 |ref| + 1e-4 rms(ref) -- one flipped bf16 rounding plus far more than the fp32 summation-order error of at most
9 * 1024 terms; an aggregate std cannot see one wrong pixel in 1e5, this can."""
import math
import re

import numpy as np
import pytest
import torch

import paramgen
from oracle import oniris_oracle as O
from test_ops_gpu import (DEV, rel, nhwc, nchw, bfr, make_bank, _conv_plain_case, _gated_conv_train_case, _conv_epilogues_case,
                          _one_frame_splitk_case, _kept_context_product_case)
from test_verification_gpu import (TIGHT, sd, packed_weight, _conv_plain_bf16_faithful_case, _gated_forward_bf16_faithful_case,
                                   _gated_backward_bf16_faithful_case, _gated_backward_epilogues_bf16_faithful_case,
                                   _one_frame_bf16_faithful_case, _gated_wgrad_integer_exact_case, _plain_wgrad_integer_exact_case)

pytestmark = pytest.mark.gpu
F = torch.nn.functional


# ---------------------------------------------------------------------------------------------------------------------
# dispatch census helpers

class Census:
    """Snapshots of the running dispatch census at named points of a test body (the `mark` argument of the case helpers)."""

    def __init__(self):
        self.at = {}

    def mark(self, name):
        from autoregressive_diffusion_amd import ops
        self.at[name] = ops.census_peek()

    def between(self, a, b):
        """{instantiation: launches} noted after mark a and up to mark b."""
        ca, cb = self.at[a], self.at[b]
        return {k: n - ca.get(k, 0) for k, n in cb.items() if n - ca.get(k, 0) > 0}


_KEY = re.compile(r"^(\w+)(?:<(.*)>)?(?: \[(.*)\])?$")


def family(key):
    """A census key ('conv_fwd_kernel<2, 9, 32, 2, true, 16, 4, false> [nt-stores]': demangled, positional) in the spelling of the
    KernelProfile keys of ops._conv_launch / ops._wgrad_launch_group; None for kernels that are not 3x3 conv families."""
    m = _KEY.match(key)
    if not m:
        return None
    name, args = m.group(1), [a.strip() for a in (m.group(2) or "").split(",") if a.strip()]
    b = lambda s: int(s == "true")
    if name == "conv_fwd_kernel":           # <S, TAPS, CK, NT, HAS_CTX, PW, NW, ACTB>
        return f"conv_fwd_kernel<S={args[0]},TAPS={args[1]},CK={args[2]},NT={args[3]},CTX={b(args[4])},PW={args[5]}>"
    if name == "conv_glds_kernel":          # <NT, PW, NW, MT, WC, CTX, RES>
        return f"conv_glds_kernel<NT={args[0]},PW={args[1]},NW={args[2]},MT={args[3]},WC={args[4]},CTX={b(args[5])}>"
    if name == "conv_stream_kernel":        # <ALIAS>
        return f"conv_stream_kernel<ALIAS={b(args[0])}>"
    if name == "conv_wgrad_glds_kernel":    # <CT, IT, NG, PW>
        return f"conv_wgrad_glds_kernel<CT={args[0]},IT={args[1]},NG={args[2]},PW={args[3]}>"
    if name == "conv_wgrad_kernel":         # <TAPS, PW, CT, IT>
        return f"conv_wgrad_kernel<TAPS={args[0]},PW={args[1]},CT={args[2]},IT={args[3]}>"
    if name == "conv_wgrad_stream_kernel":  # <PH> (4x16- or 8x16-pixel tiles; the profile key does not carry it)
        return f"conv_wgrad_stream_kernel<PH={args[0]}>"
    if name == "conv_plain_stream_kernel":
        return name
    if name.startswith("conv_eval1_kernel"):
        return f"conv_eval1_kernel<{args[0]}>"
    return None


def families(diff):
    return {f for f in (family(k) for k in diff) if f is not None}


# what a row is aimed at -> predicate over the spelling above
AIM = {
    "staged16": lambda f: f.startswith("conv_fwd_kernel<") and f.endswith("PW=16>"),
    "staged8": lambda f: f.startswith("conv_fwd_kernel<") and f.endswith("PW=8>"),
    "staged4": lambda f: f.startswith("conv_fwd_kernel<") and f.endswith("PW=4>"),
    "staged2": lambda f: f.startswith("conv_fwd_kernel<") and f.endswith("PW=2>"),
    "glds16": lambda f: f.startswith("conv_glds_kernel<") and ",PW=16," in f,
    "stream": lambda f: f.startswith("conv_stream_kernel<"),
    "plain_stream": lambda f: f == "conv_plain_stream_kernel",
    "wglds16": lambda f: f.startswith("conv_wgrad_glds_kernel<") and f.endswith("PW=16>"),
    "wreg16": lambda f: f.startswith("conv_wgrad_kernel<TAPS=9,PW=16,"),
    "wreg8": lambda f: f.startswith("conv_wgrad_kernel<TAPS=9,PW=8,"),
    "wreg4": lambda f: f.startswith("conv_wgrad_kernel<TAPS=9,PW=4,"),
    "wreg2": lambda f: f.startswith("conv_wgrad_kernel<TAPS=9,PW=2,"),
    "wstream4": lambda f: f == "conv_wgrad_stream_kernel<PH=4>",
    "wstream8": lambda f: f == "conv_wgrad_stream_kernel<PH=8>",
}
_FWD_NAMES = ("conv_fwd_kernel", "conv_glds_kernel", "conv_stream_kernel", "conv_plain_stream_kernel")
_WGRAD_NAMES = ("conv_wgrad_glds_kernel", "conv_wgrad_kernel", "conv_wgrad_stream_kernel")


def assert_aimed(cs, aims, what):
    """aims = (forward, data gradient, weight gradient).  The forward launch (between marks 'start' and 'fwd') is of the family the row
    is aimed at and of no other conv family; the backward (up to 'bwd') launched the aimed data-gradient family (it swaps Cin and
    Cout, so it can be another family than the forward: a 32 -> 24 streaming forward has a register-staged 24 -> 32 dgrad) and
    the aimed weight-gradient family, and no other."""
    fwd_aim, dgrad_aim, wgrad_aim = aims
    fwd = {f for f in families(cs.between("start", "fwd")) if f.startswith(_FWD_NAMES)}
    assert fwd and all(AIM[fwd_aim](f) for f in fwd), (what, "forward aimed at", fwd_aim, "launched", sorted(fwd))
    bwd = families(cs.between("fwd", "bwd"))
    dg = {f for f in bwd if f.startswith(_FWD_NAMES)}
    assert dg and all(AIM[dgrad_aim](f) for f in dg), (what, "data gradient aimed at", dgrad_aim, "launched", sorted(dg))
    wg = {f for f in bwd if f.startswith(_WGRAD_NAMES)}
    assert wg and all(AIM[wgrad_aim](f) for f in wg), (what, "weight gradient aimed at", wgrad_aim, "launched", sorted(wg))
    return fwd


def s2ctx_label(f):
    """ops._s2ctx_family's name for a forward family of the DART training layout."""
    if f.startswith("conv_stream_kernel"):
        return "stream"
    if f.startswith("conv_glds_kernel"):
        return "glds16" if ",PW=16," in f else "glds8"
    return "staged"


def assert_elementwise(got, ref, what):
    """|got - ref| <= 2^-7 |ref| + 1e-4 rms(ref) for every element (module docstring)."""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    rms = ref.pow(2).mean().sqrt()
    excess = (got - ref).abs() - (2.0 ** -7 * ref.abs() + 1e-4 * rms)
    n_bad = int((excess > 0).sum())
    print(what, "element-wise: worst |got - ref| - bound", float(excess.max()), "rms(ref)", float(rms), "elements over the bound", n_bad,
          "of", ref.numel())
    assert n_bad == 0, (what, n_bad, float(excess.max()))


# ---------------------------------------------------------------------------------------------------------------------
# 1. conv kernels: plain 3x3

# (N, H, W, cin, cout), (forward, data-gradient, weight-gradient) family, density of the integer-exact inputs
PLAIN = [
    # staged 8x16 tiles, nty = 1, ntx = 2, odd N, ragged channels
    ((5, 8, 32, 48, 40), ("staged16", "staged16", "wglds16"), 0.2),
    # staged, nty = 3, ntx = 1, two channel tiles per wave
    ((3, 24, 16, 64, 96), ("staged16", "staged16", "wglds16"), 0.15),
    # even N and Cin % 32 == 0 but H % 16 != 0: the LDS-DMA kernel must decline
    ((6, 24, 16, 64, 64), ("staged16", "staged16", "wglds16"), 0.12),
    # LDS-DMA plain kernel, ntx != nty in both directions
    ((4, 32, 16, 32, 64), ("glds16", "glds16", "wglds16"), 0.15),
    ((4, 16, 48, 64, 32), ("glds16", "glds16", "wglds16"), 0.12),
    # PW = 8 with nty = 2, 3 and a ragged frame pair
    ((5, 16, 8, 96, 32), ("staged8", "staged8", "wreg8"), 0.2),
    ((4, 24, 8, 64, 64), ("staged8", "staged8", "wreg8"), 0.15),
    # PW = 4 (8 frames per tile at 4x4; here nty > 1)
    ((9, 8, 4, 64, 64), ("staged4", "staged4", "wreg4"), 0.25),
    ((3, 12, 4, 32, 40), ("staged4", "staged4", "wreg4"), 0.3),
    # PW = 2
    ((33, 4, 2, 64, 64), ("staged2", "staged2", "wreg2"), 0.3),
    ((5, 6, 2, 32, 32), ("staged2", "staged2", "wreg2"), 0.4),
    # plain streaming kernel at its 512-tile threshold, an odd frame count and ragged Cout
    ((256, 8, 32, 32, 32), ("plain_stream", "plain_stream", "wglds16"), 0.05),
    ((171, 24, 16, 32, 24), ("plain_stream", "staged16", "wglds16"), 0.05),
]
_ids = lambda rows: ["x".join(str(v) for v in r[0]) for r in rows]


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("row", PLAIN, ids=_ids(PLAIN))
def test_plain_conv_vs_oracle(row):
    """Forward, data gradient and weight gradient against the fp32 oracle (body and bounds of test_conv_plain), in the family aimed at."""
    (N, H, W, cin, cout), aims, _ = row
    cs = Census()
    _conv_plain_case(N, H, W, cin, cout, 3, mark=cs.mark)
    fwd = assert_aimed(cs, aims, row[0])
    if aims[0] != "glds16":
        assert not any(f.startswith("conv_glds_kernel") for f in families(cs.between("start", "bwd"))), (row[0], fwd)


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("row", PLAIN, ids=_ids(PLAIN))
def test_plain_conv_bf16_faithful(row):
    """Forward (body of test_conv_plain_bf16_faithful) and data gradient on the operands the kernels multiply, results rounded to
    bf16: the aggregate criterion TIGHT and the element-wise bound."""
    from autoregressive_diffusion_amd import ops
    (N, H, W, cin, cout), *_ = row
    got, ref = _conv_plain_bf16_faithful_case(N, H, W, cin, cout, 3)
    assert_elementwise(got, ref, ("plain forward", row[0]))
    torch.manual_seed(19 + cin + H)
    p = torch.nn.Parameter(torch.randn(cout, cin, 3, 3).to(DEV))
    bank, (pw,) = make_bank([p])
    bank.prepare(training=True)
    w = packed_weight(pw, cout, cin, (3, 3)).double()
    x0, g0 = bfr(torch.randn(N, cin, H, W)), bfr(torch.randn(N, cout, H, W))
    x = nhwc(x0).requires_grad_(True)
    ops.conv(x, pw).backward(nhwc(g0))
    dx_ref = bfr(F.conv_transpose2d(g0.double(), w, padding=1).float())
    e = sd(nchw(x.grad), dx_ref)
    print("conv_plain dgrad bf16-faithful", row[0], e)
    assert e <= TIGHT
    assert_elementwise(nchw(x.grad), dx_ref, ("plain dgrad", row[0]))


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("row", PLAIN, ids=_ids(PLAIN))
def test_plain_conv_weight_gradient_integer_exact(row):
    """Sparse ternary x and dy: every slab entry is a small integer, a lost or misplaced position shows at full size (body and
    bounds of test_plain_conv_weight_gradient_integer_exact)."""
    (N, H, W, cin, cout), aims, dens = row
    cs = Census()
    _plain_wgrad_integer_exact_case(N, H, W, cin, cout, 3, dens, mark=cs.mark)
    assert_aimed(cs, aims, row[0])


# ---------------------------------------------------------------------------------------------------------------------
# 1. conv kernels: gated training layout

# (B, T, H, W, cin, cout), (forward, data-gradient, weight-gradient) family, density
GATED = [
    # streaming forward and weight gradient (4x16-pixel tiles); several segments; odd nty.  The dgrad is a conv with Cin and Cout
    # swapped: streaming too for 32 -> 32; for Cout = 24 / 8 it has 24 / 8 input channels and falls to the register-staged kernel
    ((2, 5, 8, 16, 32, 32), ("stream", "stream", "wstream4"), 0.2),
    ((1, 19, 8, 32, 32, 24), ("stream", "staged16", "wstream4"), 0.1),
    ((1, 9, 24, 16, 32, 8), ("stream", "staged16", "wstream4"), 0.12),
    # more 4x16-pixel tiles (9 * 2 * 32 = 576) than the 512 slabs of a weight: the weight gradient's 8x16-pixel form, nty = 16, ntx = 2
    ((9, 2, 128, 32, 32, 32), ("stream", "stream", "wstream8"), 0.04),
    # LDS-DMA 16x16 tiles (32 -> 64: its weight gradient is the streaming kernel's while the weights own enough slabs)
    ((2, 3, 16, 32, 64, 96), ("glds16", "glds16", "wglds16"), 0.1),
    ((1, 4, 32, 16, 32, 64), ("glds16", "glds16", "wstream4"), 0.12),
    ((1, 3, 48, 16, 128, 64), ("glds16", "glds16", "wglds16"), 0.1),
    # H % 16 != 0: the staged kernel (no clip report: the mp_sum backward writes a masked copy)
    ((1, 4, 24, 16, 64, 64), ("staged16", "staged16", "wglds16"), 0.12),
    # PW = 8, not the 8x8 LDS-DMA form
    ((2, 3, 16, 8, 64, 128), ("staged8", "staged8", "wreg8"), 0.15),
    ((1, 5, 24, 8, 32, 64), ("staged8", "staged8", "wreg8"), 0.15),
    # PW = 4 and PW = 2
    ((1, 8, 8, 4, 32, 64), ("staged4", "staged4", "wreg4"), 0.25),
    ((2, 3, 4, 2, 64, 64), ("staged2", "staged2", "wreg2"), 0.4),
]


def _assert_gated_aim(cs, row):
    from autoregressive_diffusion_amd import ops
    (B, T, H, W, cin, cout), aims, _ = row
    fwd = assert_aimed(cs, aims, row[0])
    mirror = ops._s2ctx_family(T, H, W, cin, ops.roundup(cin, 64), ops.roundup(cout, 32), T, (-2, -1), 1.0)
    assert {s2ctx_label(f) for f in fwd} == {mirror}, (row[0], "ops._s2ctx_family says", mirror, "the library launched", sorted(fwd))
    return mirror


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("epi", ["none", "silu", "mpsum", "mpsum_clipped"])
@pytest.mark.parametrize("row", GATED, ids=_ids(GATED))
def test_gated_conv_vs_oracle(row, epi):
    """Forward, data gradient, both weight gradients, gate (and epilogue) gradients against the fp32 oracle: bodies and bounds of
    test_gated_conv_train (no epilogue) and test_conv_epilogues (emb-scale + silu; private mp_sum with the +-256 clip armed, not
    reached and reached), in the family aimed at."""
    (B, T, H, W, cin, cout), *_ = row
    cs = Census()
    if epi == "none":
        _gated_conv_train_case(B, T, H, W, cin, cout, mark=cs.mark)
        mirror = _assert_gated_aim(cs, row)
    else:
        from autoregressive_diffusion_amd import ops
        mirror = ops._s2ctx_family(T, H, W, cin, ops.roundup(cin, 64), ops.roundup(cout, 32), T, (-2, -1), 1.0)
        cfg = ("emb_silu", False) if epi == "silu" else ("mpsum", True)
        _conv_epilogues_case(True, H, W, cout, epi == "mpsum_clipped", B=B, T=T, cin=cin, configs=(cfg,),
                             expect_alias=mirror != "staged" and ops.roundup(cout, 8) <= 512, mark=cs.mark)
        assert _assert_gated_aim(cs, row) == mirror
    print("gated", row[0], epi, "family", mirror)


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("epi", ["none", "mpsum", "silu"])
@pytest.mark.parametrize("row", GATED, ids=_ids(GATED))
def test_gated_conv_forward_bf16_faithful(row, epi):
    (B, T, H, W, cin, cout), *_ = row
    got, ref = _gated_forward_bf16_faithful_case(B, T, H, W, cin, cout, epi)
    if epi != "silu":                      # (fast sigmoid: the aggregate criterion only)
        assert_elementwise(got, ref, ("gated forward", row[0], epi))


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("epi", ["none", "mpsum", "mpsum_clipped", "silu"])
@pytest.mark.parametrize("row", GATED, ids=_ids(GATED))
def test_gated_conv_backward_bf16_faithful(row, epi):
    (B, T, H, W, cin, cout), *_ = row
    if epi == "none":
        dx, dx_ref = _gated_backward_bf16_faithful_case(B, T, H, W, cin, cout)
    else:
        dx, dx_ref = _gated_backward_epilogues_bf16_faithful_case(B, T, H, W, cin, cout, epi)
    if epi in ("none", "mpsum"):           # linear epilogues (the clip never reached)
        assert_elementwise(dx, dx_ref, ("gated dgrad", row[0], epi))


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("row", GATED, ids=_ids(GATED))
def test_gated_conv_weight_gradient_integer_exact(row):
    (B, T, H, W, cin, cout), _, dens = row
    cs = Census()
    _gated_wgrad_integer_exact_case(B, T, H, W, cin, cout, dens, mark=cs.mark)
    _assert_gated_aim(cs, row)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the Python mirrors of the C dispatch

def _run_fwd_bwd(kind, shape):
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(1)
    if kind == "plain":
        N, H, W, cin, cout = shape
        p = torch.nn.Parameter(torch.randn(cout, cin, 3, 3).to(DEV))
        bank, (pw,) = make_bank([p])
        bank.prepare(training=True)
        x = nhwc(torch.randn(N, cin, H, W)).requires_grad_(True)
        y = ops.conv(x, pw)
    else:
        B, T, H, W, cin, cout = shape
        N = B * 2 * T
        p2, p3 = torch.nn.Parameter(torch.randn(cout, cin, 3, 3).to(DEV)), torch.nn.Parameter(torch.randn(cout, cin, 2, 3, 3).to(DEV))
        bank, (pw2, pw3) = make_bank([p2, p3])
        bank.prepare(training=True)
        x = nhwc(torch.randn(N, cin, H, W)).requires_grad_(True)
        g = (torch.rand(N) * 0.6 + 0.05).to(DEV).requires_grad_(True)
        y = ops.gated_conv_train(x, g, pw2, pw3, B, T)
    y.backward(torch.randn_like(y))
    bank.backward()
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind,row", [("plain", r) for r in PLAIN] + [("gated", r) for r in GATED],
                         ids=["plain-" + i for i in _ids(PLAIN)] + ["gated-" + i for i in _ids(GATED)])
def test_python_mirrors_name_the_launched_family(kind, row):
    """ops._conv_launch and ops._wgrad_launch_group restate the C dispatch by hand to name a launch for KernelProfile (bench.py's
    roofline table): forward, data gradient and weight gradient of every row under KernelProfile, its keys against the census of
    the same launches."""
    from autoregressive_diffusion_amd import ops
    before = ops.census_peek()
    ops.KernelProfile.start()
    try:
        _run_fwd_bwd(kind, row[0])
    finally:
        agg = ops.KernelProfile.stop()
    after = ops.census_peek()
    launched = families({k: n - before.get(k, 0) for k, n in after.items() if n - before.get(k, 0) > 0})
    launched = {re.sub(r"^(conv_wgrad_stream_kernel)<PH=\d>$", r"\1", f) for f in launched if f.startswith(_FWD_NAMES + _WGRAD_NAMES)}
    named = {k for k in agg if k.startswith(_FWD_NAMES + _WGRAD_NAMES)}
    print(kind, row[0], "launched", sorted(launched), "named", sorted(named))
    assert launched and named == launched, (row[0], "KernelProfile names", sorted(named - launched), "the library launched", sorted(launched - named))


# ---------------------------------------------------------------------------------------------------------------------
# 1. forced variants: 8-wave staged tiles (big_tile 1 / 2), register-staged weight gradient

@pytest.mark.parametrize("knob,value,aims", [("BIG_TILE", 2, ("staged16", "staged16", "wglds16")),
                                             ("WGRAD_VARIANT", -1, ("glds16", "glds16", "wreg16"))], ids=["big_tile=2", "wgrad_variant=-1"])
@pytest.mark.parametrize("H,W", [(16, 32), (32, 16)])
def test_forced_conv_variants(H, W, knob, value, aims, monkeypatch):
    """The variants a knob forces (OnirisConvArgs.big_tile = 2: the 8-wave 16x16 register-staged tiles -- big_tile = 1 takes them only
    from 256 workgroups on, which no oracle-sized input reaches; OnirisWgradArgs.pad_ < 0: the register-staged weight gradient) on
    16x32 and 32x16, oracle and integer-exact weight gradient."""
    from autoregressive_diffusion_amd import ops
    monkeypatch.setattr(ops, knob, value)
    B, T, cin, cout = 2, 3, 64, 64
    row = ((B, T, H, W, cin, cout), aims, 0.12)
    cs = Census()
    _gated_conv_train_case(B, T, H, W, cin, cout, mark=cs.mark)
    _assert_gated_aim(cs, row)
    if knob == "BIG_TILE":
        nw = {k for k in cs.between("start", "fwd") if k.startswith("conv_fwd_kernel<")}
        assert nw and all("16, 8," in k for k in nw), nw          # <.., PW = 16, NW = 8, ..>
    cs = Census()
    _gated_wgrad_integer_exact_case(B, T, H, W, cin, cout, 0.12, mark=cs.mark)
    _assert_gated_aim(cs, row)


# ---------------------------------------------------------------------------------------------------------------------
# 1. one-frame cached evaluation (csrc/conv_eval1.h: H % 8 == 0, W % 8 == 0) and its split-K fallback

@pytest.mark.parametrize("B,H,W,cin,cout", [(2, 8, 16, 128, 128), (1, 16, 8, 256, 256), (3, 24, 16, 64, 64), (1, 24, 16, 32, 32)])
def test_one_frame_conv_bf16_faithful(B, H, W, cin, cout):
    got, ref = _one_frame_bf16_faithful_case(B, H, W, cin, cout)
    assert_elementwise(got, ref, ("one-frame gated conv", (B, H, W, cin, cout)))


@pytest.mark.parametrize("kernel", ["eval1", "eval1<32>", "staged"])
@pytest.mark.parametrize("B,H,W,cin,cout,epi", [(1, 8, 16, 256, 256, "silu"), (1, 16, 8, 128, 128, "mpsum"), (2, 24, 16, 64, 64, "none"),
                                                (3, 24, 16, 32, 32, "mpsum"), (1, 16, 8, 96, 160, "silu")])
def test_one_frame_conv_splitk(B, H, W, cin, cout, epi, kernel, monkeypatch):
    """Body of test_gated_conv_eval_one_frame_splitk.  eval1: the weight-streaming kernel (16- and, big_tile bit 256, 32-channel
    workgroups); staged: big_tile bit 16 switches it off and the launch falls back to the register-staged kernel, whose K loop is
    split over workgroups when ops.SPLITK lends the workspace."""
    from autoregressive_diffusion_amd import ops
    bits = {"eval1": 0, "eval1<32>": 256, "staged": 16}[kernel]
    monkeypatch.setattr(ops, "BIG_TILE", ops.BIG_TILE | bits)
    cs = Census()
    _one_frame_splitk_case(B, H, W, cin, cout, epi, monkeypatch, mark=cs.mark)
    for a, b in (("splitk=1", "splitk=0"), ("splitk=0", "end")):
        fam = {f for f in families(cs.between(a, b)) if f.startswith(("conv_fwd_kernel", "conv_eval1_kernel"))}
        if kernel == "staged":
            assert fam and all(f.startswith("conv_fwd_kernel<S=1,TAPS=9,") and f.endswith(f"CTX=1,PW={16 if W >= 16 else W}>") for f in fam), fam
        else:
            want = {"conv_eval1_kernel<32>"} if kernel == "eval1<32>" or (ops.roundup(cout, 32) // 32) * (W // 8) * (H // 8) * B > 128 \
                else {"conv_eval1_kernel<16>"}
            assert fam == want, (fam, want)


@pytest.mark.parametrize("B,H,W,cin,cout,epi", [(1, 8, 16, 256, 256, "silu"), (2, 16, 8, 128, 128, "mpsum"), (3, 24, 16, 64, 64, "none"),
                                                (1, 24, 16, 96, 160, "mpsum"), (2, 8, 16, 32, 32, "silu")])
def test_one_frame_conv_kept_context_product(B, H, W, cin, cout, epi):
    """ctx_prod_mode 1 (store), 3 (context phases only), 2 (read): body of test_one_frame_conv_kept_context_product."""
    _kept_context_product_case(B, H, W, cin, cout, epi)


# ---------------------------------------------------------------------------------------------------------------------
# 1. 1x1 convs (position-linear kernels: this checks the wrappers)

@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("N,H,W,cin,cout", [(3, 6, 10, 64, 96), (5, 24, 16, 128, 64), (22, 24, 16, 64, 192)])      # (the last: >= 8192 positions, LDS-DMA GEMM)
def test_conv1x1(N, H, W, cin, cout):
    _conv_plain_case(N, H, W, cin, cout, 1)


@pytest.mark.parametrize("N,H,W,C1,C2,cout", [(1, 6, 10, 64, 32, 64), (2, 24, 16, 128, 64, 128)])
def test_conv_cat_act_vs_oracle(N, H, W, C1, C2, cout):
    """ops.conv_cat_act (mp_cat + mp_silu + the 1x1 skip conv of the concatenation, one launch) against the oracle primitives."""
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(N + H + C1)
    w0 = O.normalize(O.normalize(torch.randn(cout, C1 + C2, 1, 1)))
    p = torch.nn.Parameter(w0.clone().to(DEV))
    bank, (pw,) = make_bank([p])
    bank.prepare(training=False)
    x0, s0 = bfr(torch.randn(N, C1, H, W) * 1.5), bfr(torch.randn(N, C2, H, W))
    w1, w2 = 0.83, 1.21
    with torch.no_grad():
        assert ops.conv_cat_act_ok(nhwc(x0), nhwc(s0), pw)
        y, a = ops.conv_cat_act(nhwc(x0), nhwc(s0), w1, w2, pw)
    xo = torch.cat([w1 * x0, w2 * s0], 1)
    w_eff, _ = O.weight_effective(w0, 1.0, False)
    e = (rel(nchw(y)[:, :cout], F.conv2d(xo, w_eff)), rel(nchw(a), O.mp_silu(xo)))
    print("conv_cat_act", (N, H, W, C1, C2, cout), "rel y / a", e)
    assert max(e) < 1e-2


# ---------------------------------------------------------------------------------------------------------------------
# 3. element-wise kernels that index rows and columns

EW_SHAPES = [(3, 8, 16, 64), (2, 24, 8, 32), (5, 6, 10, 48)]


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("f", [[1, 1], [1, 3, 3, 1], [1, 2, 3, 3, 2, 1]])
@pytest.mark.parametrize("N,H,W,C", EW_SHAPES)
def test_resample(N, H, W, C, f):
    """ops.resample down / up, forward and adjoint with and without a second gradient joining in the backward kernel (`dadd`),
    against O.resample; the [1, 1] filter is the fused 2x2-mean / nearest-x2 kernel (bound of test_resample_general_filter)."""
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(10 + len(f) + H)
    taps = ops.resample_taps(f)
    x0 = bfr(torch.randn(N, C, H, W))
    for mode in ("down", "up"):
        for parked in (False, True):
            x = nhwc(x0).requires_grad_(True)
            slot = ops.GradSlot() if parked else None
            y = ops.resample(x, mode, slot, taps)
            assert tuple(y.shape) == ((N, H // 2, W // 2, C) if mode == "down" else (N, 2 * H, 2 * W, C))
            g0 = bfr(torch.randn(nchw(y).shape))
            extra = bfr(torch.randn(x0.shape)) if parked else torch.zeros(x0.shape)
            if parked:
                slot.put(nhwc(extra))
            y.backward(nhwc(g0))
            xr = x0.clone().requires_grad_(True)
            yr = O.resample(xr, mode, f)
            (yr * g0).sum().backward()
            e = (rel(nchw(y), yr), rel(nchw(x.grad), xr.grad + extra))
            print("resample", (N, H, W, C), f, mode, "dadd" if parked else "", e)
            assert max(e) < 5e-3
    ops.GradSlot.live = []


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("mode,norm", [("down", True), ("down", False), ("up", True), ("up", False)])
@pytest.mark.parametrize("N,H,W,C", EW_SHAPES)
def test_act_with_resample_vs_oracle(N, H, W, C, mode, norm):
    """ops.act(..., resample=mode) -- the resampling inside the activation launch (Ho, Wo unpacked by hand in ops._ActFn), its
    backward with the resample adjoint behind act_bwd and a second gradient of the un-resampled input parked in a GradSlot --
    against O.resample followed by the oracle's normalize / mp_silu (bound of test_act_fused)."""
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(12 + H)
    x0 = bfr(torch.randn(N, C, H, W) * 1.3)
    extra = bfr(torch.randn(N, C, H, W))
    x = nhwc(x0).requires_grad_(True)
    slot = ops.GradSlot()
    if norm and (C // 8) & (C // 8 - 1):          # the pixel norm is written for C / 8 = 2^k lanes per pixel: C = 48 is refused, not miscomputed
        with pytest.raises(ops.OnirisError, match="pixel norm"):
            ops.act(x, norm=norm, want_xo=True, in_slot=slot, resample=mode)
        ops.GradSlot.live = []
        return
    xo, a = ops.act(x, norm=norm, want_xo=True, in_slot=slot, resample=mode)
    Ho, Wo = (H // 2, W // 2) if mode == "down" else (2 * H, 2 * W)
    assert tuple(xo.shape) == tuple(a.shape) == (N, Ho, Wo, C)
    ga0, gx0 = bfr(torch.randn(N, C, Ho, Wo)), bfr(torch.randn(N, C, Ho, Wo))
    slot.put(nhwc(extra))
    ((a.float() * nhwc(ga0).float()).sum() + (xo.float() * nhwc(gx0).float()).sum()).backward()
    assert slot.g is None
    xr = x0.clone().requires_grad_(True)
    v = O.resample(xr, mode)
    if norm:
        v = O.normalize(v, dim=1)
    ar = O.mp_silu(v)
    ((ar * ga0).sum() + (v * gx0).sum()).backward()
    e = (rel(nchw(xo), v), rel(nchw(a), ar), rel(nchw(x.grad), xr.grad + extra))
    print("act + resample", (N, H, W, C), mode, "norm" if norm else "", "rel xo / a / dx", e)
    assert max(e) < 1e-2
    ops.GradSlot.live = []


@pytest.mark.parametrize("C", [4, 8])
@pytest.mark.parametrize("H,W", [(16, 24), (24, 16)])
def test_dart_passes(H, W, C):
    """oniris_dart_input / dart_loss / dart_loss_bwd / precond_out / dart_input_pair (csrc/elementwise.hip: one index H*W, frames in
    NCHW fp32 on one side and channels-last bf16 on the other) against the torch formulas (loss.py:17-47, networks_edm2.py:278-297)."""
    from autoregressive_diffusion_amd import ops
    g = torch.Generator().manual_seed(H + C)
    B, T, S, sdv = 2, 3, 2, 0.7
    images = torch.randn(B, T, C, H, W, generator=g)
    noise = torch.randn(B, S * T, C, H, W, generator=g)
    sigma = (torch.randn(B, S * T, generator=g) * 0.8).exp()
    dimg, dnoise, dsig = images.to(DEV), noise.to(DEV), sigma.to(DEV)
    x = torch.cat([images, images], 1) + sigma[:, :, None, None, None] * noise                    # (B, S*T, C, H, W)
    cin = 1 / (sdv ** 2 + sigma ** 2).sqrt()
    # packed input
    xcl, cn = ops.dart_input(dimg, dnoise, dsig, S, sdv, want_c_noise=True)
    want_in = (cin[:, :, None, None, None] * x).reshape(B * S * T, C, H, W).permute(0, 2, 3, 1)
    assert tuple(xcl.shape) == (B * S * T, H, W, ops.IN_PAD)
    assert rel(xcl[..., :C], want_in) < 4e-3                                                      # (bf16 output rounding)
    assert torch.equal(xcl[..., C].float().cpu(), torch.ones(B * S * T, H, W)) and float(xcl[..., C + 1:].abs().max()) == 0.0
    assert torch.allclose(cn.cpu(), sigma.log() / 4, atol=1e-6, rtol=1e-6)
    # loss and its backward
    Fcl0 = torch.zeros(B * S * T, H, W, 8)
    Fcl0[..., :C] = torch.randn(B * S * T, H, W, C, generator=g)
    Fcl0 = bfr(Fcl0)
    Fcl = Fcl0.to(DEV, torch.bfloat16).requires_grad_(True)
    og = torch.tensor(0.7, device=DEV, requires_grad=True)
    losses = ops.dart_loss(Fcl, og, dimg, dnoise, dsig, S, sdv)
    gl = torch.rand(B, T, generator=g) + 0.5
    (losses * gl.to(DEV)).sum().backward()
    Fr = Fcl0[..., :C].double().requires_grad_(True)
    ogr = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    sg = sigma[:, T:].double()
    den = sg ** 2 + sdv ** 2
    Fn = Fr.permute(0, 3, 1, 2).reshape(B, S * T, C, H, W)[:, T:]
    D = (sdv ** 2 / den)[:, :, None, None, None] * x[:, T:].double() + (sg * sdv / den.sqrt())[:, :, None, None, None] * (Fn * ogr)
    lr = ((D - images.double()) ** 2).mean(dim=(-1, -2, -3))
    (lr * gl.double()).sum().backward()
    # one block's fp32 sum of C*H*W <= 3072 non-negative terms: a few ulp; a lost pixel would be 1 / (H W) = 2.6e-3
    assert torch.allclose(losses.double().cpu(), lr.detach(), rtol=1e-5, atol=0), (losses.cpu(), lr)
    dF = Fcl.grad.float().cpu()
    assert rel(dF[..., :C], Fr.grad) < 4e-3 and (C == 8 or float(dF[..., C:].abs().max()) == 0.0)   # (bf16 store; zero for the clean half and the pad)
    assert float(dF.reshape(B, S, T, -1)[:, 0].abs().max()) == 0.0
    assert abs(float(og.grad) - float(ogr.grad)) <= 1e-4 * abs(float(ogr.grad)) + 1e-6
    # output side in eval
    xe = torch.randn(B, T, C, H, W, generator=g)
    se = (torch.randn(B, T, generator=g) * 0.8).exp()
    Fe0 = torch.zeros(B * T, H, W, 8)
    Fe0[..., :C] = torch.randn(B * T, H, W, C, generator=g)
    Fe0 = bfr(Fe0)
    Dg = ops.precond_out(Fe0.to(DEV, torch.bfloat16), xe.to(DEV), se.to(DEV), og.detach(), sdv)
    dene = se ** 2 + sdv ** 2
    wantD = (sdv ** 2 / dene)[:, :, None, None, None] * xe + \
        (se * sdv / dene.sqrt())[:, :, None, None, None] * (Fe0[..., :C].permute(0, 3, 1, 2).reshape(B, T, C, H, W) * 0.7)
    assert torch.allclose(Dg.cpu(), wantD, atol=1e-5, rtol=1e-5)
    # guided pair input: rows [B*t, 2*B*t) repeat rows [0, B*t)
    xp, cnp = ops.dart_input_pair(xe.to(DEV), se.to(DEV), sdv)
    cine = 1 / (sdv ** 2 + se ** 2).sqrt()
    want_p = (cine[:, :, None, None, None] * xe).reshape(B * T, C, H, W).permute(0, 2, 3, 1)
    assert tuple(xp.shape) == (2 * B * T, H, W, ops.IN_PAD) and torch.equal(xp[:B * T], xp[B * T:])
    assert rel(xp[:B * T, ..., :C], want_p) < 4e-3 and torch.equal(xp[..., C].float().cpu(), torch.ones(2 * B * T, H, W))
    assert float(xp[..., C + 1:].abs().max()) == 0.0 and torch.allclose(cnp.cpu(), se.log() / 4, atol=1e-6, rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# 4. modules and whole steps

def _attn_params(C, video, seed):
    shapes = {"attn_qkv.weight.weight": (3 * C, C, 1, 1), "attn_proj.weight.weight": (C, C, 1, 1)}
    if video:
        shapes.update({"rope.inv_freq": (32,), "rope.scale": (32,)})
    return paramgen.prenormalise(paramgen.fill(shapes, seed))


def _load(mod, params):
    mod.load_state_dict({k: v.clone() for k, v in params.items()}, strict=True)
    return mod.to(DEV)


@pytest.mark.parametrize("kind,B,T,H,W,m", [("frame", 5, 1, 8, 16, 2), ("frame", 6, 1, 16, 8, 1), ("frame", 3, 1, 8, 4, 1),
                                            ("video", 1, 2, 8, 16, 1), ("video", 2, 2, 16, 8, 2), ("video", 1, 8, 8, 4, 2)])
def test_attention_modules(kind, B, T, H, W, m):
    """FrameAttention / VideoAttention modules (qkv conv, normalisation, rotary embedding, attention, projection, mp_sum) forward and
    every gradient against the oracle, P = H * W = 128 (the fused frame qkv kernels of csrc/attention_frame.h) and P = 32 (T = 8);
    bounds of test_g6_attention_modules."""
    from edm2.attention import VideoAttention, FrameAttention
    C = 64 * m
    N = B * 2 * T if kind == "video" else B
    p = _attn_params(C, kind == "video", 40 + H + m)
    att = _load(VideoAttention(C, m) if kind == "video" else FrameAttention(C, m), p).train()
    g = torch.Generator().manual_seed(H * W + m)
    x0, gy0 = torch.randn(N, C, H, W, generator=g), torch.randn(N, C, H, W, generator=g)
    x = x0.clone().to(DEV).requires_grad_(True)
    cs = Census()
    cs.mark("start")
    y, _ = att(x, B) if kind == "video" else att(x)
    y.backward(gy0.to(DEV))
    cs.mark("end")
    pr = {"a." + k: v.clone().requires_grad_(v.is_floating_point() and "rope" not in k) for k, v in p.items()}
    xr = x0.clone().requires_grad_(True)
    if kind == "video":
        yr, _ = O.video_attention(pr, "a.", xr, B, m, None, False, False, True)
    else:
        yr = O.frame_attention(pr, "a.", xr, m, True)
    (yr * gy0).sum().backward()
    e = dict(y=rel(y, yr), gx=rel(x.grad, xr.grad), g_qkv=rel(att.attn_qkv.weight.weight.grad, pr["a.attn_qkv.weight.weight"].grad),
             g_proj=rel(att.attn_proj.weight.weight.grad, pr["a.attn_proj.weight.weight"].grad))
    print("attention module", (kind, B, T, H, W, m), e)
    assert e["y"] < 1e-2 and e["gx"] < 2e-2 and e["g_qkv"] < 3e-2 and e["g_proj"] < 3e-2
    if kind == "frame" and H * W == 128:
        seen = cs.between("start", "end")
        assert any(k.startswith("frame_attn_qkv_fwd_kernel") for k in seen) and any(k.startswith("frame_attn_qkv_bwd_kernel") for k in seen), sorted(seen)


from test_model_gpu import CS_SMALL


def _block_case(tag, Hi, Wi, T=2, seed=71):
    """One Block (tag 'enc': down + FrameAttention, 'dec': up + VideoAttention) on an Hi x Wi input, forward and backward, HIP against
    the oracle: (errors of y / gx / gemb, rel L2 per weight gradient, gate-scalar errors own-relative and relative to the largest)."""
    from edm2.networks_edm2 import Block
    cemb = 32
    cin, cout, flavor, att, mode = (32, 64, "enc", "frame", "down") if tag == "enc" else (96, 64, "dec", "video", "up")
    Ho, Wo = (Hi // 2, Wi // 2) if tag == "enc" else (2 * Hi, 2 * Wi)
    shapes = {"emb_gain": (), "emb_linear.weight.weight": (cout, cemb)}
    shapes.update(paramgen._conv_keys("conv_res0.", cout if flavor == "enc" else cin, cout))
    shapes.update(paramgen._conv_keys("conv_res1.", cout, cout))
    shapes["conv_skip.weight.weight"] = (cout, cin, 1, 1)
    shapes["attn.attn_qkv.weight.weight"] = (3 * cout, cout, 1, 1)
    shapes["attn.attn_proj.weight.weight"] = (cout, cout, 1, 1)
    if att == "video":
        shapes["attn.rope.inv_freq"] = (32,)
        shapes["attn.rope.scale"] = (32,)
    p = paramgen.prenormalise(paramgen.fill(shapes, seed))
    e_ = dict(kind="block", name="blk", cin=cin, cout=cout, flavor=flavor, mode=mode, attention=att, heads=1)
    blk = _load(Block(cin, cout, cemb, flavor=flavor, resample_mode=mode, attention=att), p).train()
    g = torch.Generator().manual_seed(seed + 1)
    B = 1
    N = B * 2 * T
    x0, emb0, cn0 = torch.randn(N, cin, Hi, Wi, generator=g), torch.randn(N, cemb, generator=g), torch.randn(B, 2 * T, generator=g)
    gy0 = torch.randn(N, cout, Ho, Wo, generator=g)
    x, emb = x0.clone().to(DEV).requires_grad_(True), emb0.clone().to(DEV).requires_grad_(True)
    # per-frame gate gradients d loss / d gate[n] of both gated convs, on either side: the gate tensor of the HIP module (edm2/conv.py
    # hands it to ops.gated_conv_train) and the oracle's (O.gating), and the oracle's Jacobian d gate[n] / d (gating scalar)
    from autoregressive_diffusion_amd import ops
    hip_dg, ora_dg, jac = [], {}, {}
    real_gct, real_gating = ops.gated_conv_train, O.gating

    def gct(x_, gate, *a, **k):
        i = len(hip_dg)
        hip_dg.append(None)
        gate.register_hook(lambda g_: hip_dg.__setitem__(i, g_.detach().float().cpu().reshape(-1).clone()))
        return real_gct(x_, gate, *a, **k)

    def gating(p_, prefix, *a, **k):
        g_, n_ = real_gating(p_, prefix, *a, **k)
        flat = g_.reshape(-1)
        for name in ("mult", "offset", "min_gating", "max_gating"):
            th = p_[prefix + name]
            jac[prefix + name] = torch.stack([torch.autograd.grad(flat[n], th, retain_graph=True)[0].reshape(-1) for n in range(flat.numel())])
        g_.register_hook(lambda gg: ora_dg.__setitem__(prefix, gg.detach().reshape(-1).clone()))
        return g_, n_
    ops.gated_conv_train = gct
    try:
        y, _ = blk(x, emb, B, cn0.to(DEV))
    finally:
        ops.gated_conv_train = real_gct
    assert tuple(y.shape) == (N, cout, Ho, Wo)
    y.backward(gy0.to(DEV))
    pr = {"b." + k: v.clone().requires_grad_(v.is_floating_point() and "rope" not in k) for k, v in p.items()}
    xr, er = x0.clone().requires_grad_(True), emb0.clone().requires_grad_(True)
    O.gating = gating
    try:
        yr, _ = O.block_forward(pr, "b.", e_, xr, er, B, cn0, None, False, False, True)
    finally:
        O.gating = real_gating
    (yr * gy0).sum().backward()
    e = dict(y=rel(y, yr), gx=rel(x.grad, xr.grad), gemb=rel(emb.grad, er.grad))
    assert len(hip_dg) == 2 and all(h is not None for h in hip_dg) and len(ora_dg) == 2
    frames = {c: (h, ora_dg[f"b.{c}.gating."]) for c, h in zip(("conv_res0", "conv_res1"), hip_dg)}
    e["dgate"] = {c: float((h - r).norm() / r.norm()) for c, (h, r) in frames.items()}
    prm = dict(blk.named_parameters())
    wg = {k: rel(prm[k].grad, pr["b." + k].grad) for k in prm if k.endswith("weight.weight")}
    print("block", tag, (Hi, Wi), "T", T, e, "worst weight gradient", max(wg, key=wg.get), max(wg.values()))
    sc = {k: (prm[k].grad.detach().float().cpu().reshape(-1), pr["b." + k].grad.reshape(-1)) for k in prm
          if "gating" in k and prm[k].grad is not None and pr["b." + k].grad is not None}
    assert len(sc) >= 8, sorted(sc)
    top = max(float(r.abs().max()) for _, r in sc.values())
    own = {k: float((h - r).abs().max() / r.abs().max()) for k, (h, r) in sc.items() if float(r.abs().max()) >= 1e-2 * top}
    rtop = {k: float((h - r).abs().max() / top) for k, (h, r) in sc.items()}
    print("block", tag, (Hi, Wi), "T", T, "gate gradients: worst own-relative", max(own, key=own.get), max(own.values()),
          "; worst relative to the largest", max(rtop, key=rtop.get), max(rtop.values()))
    # a gating scalar's gradient is sum_n dgate[n] J[n], J[n] = d gate[n] / d theta: |error| <= |error of dgate|_2 |J|_2 (Cauchy-Schwarz),
    # so it is stated in units of |dgate|_2 |J|_2, where the per-frame bound applies to it unchanged
    terms = {}
    for k, (h, r) in sc.items():
        conv = k.split(".")[0]
        unit = frames[conv][1].norm() * jac["b." + k].norm(dim=0)
        terms[k] = float(((h - r).abs() / unit).max())
    print("block", tag, (Hi, Wi), "T", T, "per-frame gate gradients rel L2", e["dgate"], "; scalar error / (|dgate|_2 |J|_2): worst",
          max(terms, key=terms.get), max(terms.values()))
    return e, wg, own, rtop, terms


@pytest.mark.parametrize("tag,T,seed", [("enc", 2, 71), ("enc", 8, 91), ("dec", 2, 71)])
def test_blocks(tag, T, seed):
    """One Block per flavour -- encoder: 2x2-mean down to 16x8, 1x1 skip conv, pixel norm, gated convs, FrameAttention (P = 128);
    decoder: nearest-x2 up to 16x8, gated convs, skip conv, VideoAttention -- forward, input / embedding / weight gradients
    (bounds of test_g7_blocks and test_g3_gated_conv_module) and the gate gradients against the oracle, on 4 frames (T = 2) and,
    the encoder, on 16.

    Gate gradients.  What the kernels produce is d loss / d gate[n] per frame; a gating scalar's gradient is their sum over frames
    against the smooth weights d gate[n] / d theta (edm2/conv.py Gating.forward), terms of either sign.  Asserted:
      - per-frame d loss / d gate[n] of both gated convs, relative L2 over the frames, under test_gated_conv_train's bound for
        exactly this quantity (dg < 1.2e-2);
      - every gating scalar's gradient sum_n dgate[n] J[n] within that same 1.2 % of |dgate|_2 |J|_2 -- by Cauchy-Schwarz what the
        per-frame bound implies for it when the module's own gating backward adds nothing; the unit comes from the oracle's
        per-frame gradients and Jacobian alone.  (The worst instance below measures 0.77 %; relative to the sum of the magnitudes
        of its terms it measures 3.4 %, because the frame with the largest error has the largest J and the smallest gradient.)
    test_g7_blocks states gate scalars relative to their own (cancelled) sum and to the block's largest, with bounds that are twice
    what ITS fixture measured (encoder: 10 % / 0.7 %).  Those are figures of one instance, not of the kernels: measured on the
    MI355X over 40 seeds each (T = 2; profiles/nonsquare_block_gates.txt), the worst gate scalar relative to the largest has median
    0.68 % on 32x16 inputs, 0.62 % on 16x16 and 0.55 % on 32x32 (maxima 6.4 %, 5.0 %, 4.1 %), and 19, 19 and 17 of the 40
    instances exceed the fixture's bounds -- square and non-square alike.  The (T = 2, seed 71) instance kept here is the worst of
    them: per frame HIP has +54.24 -43.13 -2.17 +32.45 for conv_res1 against the oracle's +54.37 -43.13 -1.59 +32.57 (0.8 % relative
    L2, at most 1.1 % of the largest frame), and the max_gating sum of these cancels to 8.5 % of the block's largest gradient, so
    the same 0.6 absolute is 63 % of it (5.4 % of the largest).  The figures in g7's form are printed for every instance."""
    e, wg, own, rtop, terms = _block_case(tag, *((32, 16) if tag == "enc" else (8, 4)), T=T, seed=seed)
    assert e["y"] < 1e-2 and e["gx"] < 1.1e-2 and e["gemb"] < 1.3e-2
    assert max(wg.values()) < 3e-2, wg
    assert max(e["dgate"].values()) < 1.2e-2, e["dgate"]
    assert max(terms.values()) < 1.2e-2, terms


# `img_resolution` only names the levels ('32x32_conv', '16x16_down', ...): level l of an H x W input is (H >> l) x (W >> l).
# portrait 32x16: levels 32x16, 16x8 (FrameAttention, P = 128), 8x4 (VideoAttention, P = 32: T P = 256 with T = 8)
PORTRAIT = (dict(CS_SMALL, channel_mult=[1, 2, 4], video_attn_resolutions=[8], frame_attn_resolutions=[16]), 32, 16)
# landscape 16x32: two levels (4x8 is outside the 3x3 domain), 16x32 and 8x16 with VideoAttention on 64 channels, P = 128
LANDSCAPE = (dict(CS_SMALL, channel_mult=[1, 2], video_attn_resolutions=[16], frame_attn_resolutions=[]), 16, 32)

def _nonsquare_step(cfg, H, W, Tn, just_2d):
    from edm2.networks_edm2 import UNet, Precond
    from edm2.loss import EDM2Loss
    p = paramgen.prenormalise(paramgen.precond_params(cfg, 303))
    net = _load(Precond(UNet(**cfg), sigma_data=1.0), p).train()
    g = torch.Generator().manual_seed(304)
    B = 1
    images = torch.randn(B, Tn, 8, H, W, generator=g)
    sigma = (torch.randn(B, 2 * Tn, generator=g) + 0.9).exp()
    sigma[:, :Tn] = torch.rand(B, 1, generator=g) * 0.1
    eps = torch.randn(B, 2 * Tn, 8, H, W, generator=g)
    if just_2d:
        sigma, eps = sigma[:, Tn:].contiguous(), eps[:, Tn:].contiguous()
    loss, _ = EDM2Loss(P_mean=0.9, P_std=1.0, sigma_data=1.0, context_noise_reduction=0.1)(
        net, images.to(DEV), None, sigma=sigma.to(DEV), just_2d=just_2d, noise=eps.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    pr = {k: v.clone().requires_grad_(v.is_floating_point() and "rope" not in k and "fourier" not in k) for k, v in p.items()}
    ref, _, _ = O.edm2_loss(pr, cfg, images, sigma, eps, None, just_2d=just_2d, sigma_data=1.0)
    ref.backward()
    return loss, dict(net.named_parameters()), float(ref.item()), {k: (v.grad.detach().clone() if v.grad is not None else None) for k, v in pr.items()}


@pytest.mark.parametrize("mode", ["3d", "2d"])
@pytest.mark.parametrize("tag,shape", [("portrait-32x16", PORTRAIT), ("landscape-16x32", LANDSCAPE)])
def test_training_step_vs_oracle(tag, shape, mode):
    """One training step -- loss, every weight gradient, the scalar gradients -- on a non-square input against the fp32 oracle, in
    the form and under the bounds of test_cs_shaped_unet_vs_oracle (test_model_gpu._full_net_asserts)."""
    import test_model_gpu as M
    cfg, H, W = shape
    just_2d = mode == "2d"
    loss, prm, ref_loss, ref_grad = _nonsquare_step(cfg, H, W, 8, just_2d)
    live = [k for k in prm if k.endswith("weight.weight") and ref_grad.get(k) is not None and float(ref_grad[k].abs().max()) > 0]
    missing = [k for k in live if prm[k].grad is None]
    assert not missing, missing
    errs = {k: rel(prm[k].grad, ref_grad[k]) for k in live}
    M._full_net_asserts(tag, tag, loss, ref_loss, prm, ref_grad, errs, False, just_2d)       # (bounds: M.SCALAR_GRAD_BOUNDS[tag[/2d]])


def _fork(c):
    return {k: _fork(v) for k, v in c.items()} if isinstance(c, dict) else c


@pytest.mark.parametrize("guidance", [1.0, 1.5])
def test_cached_rollout_frame_vs_oracle(guidance):
    """A 4-frame causal prefill and one generated frame of the portrait net (32x16: KV ring and kept context products with
    P = H * W = 128 / 32 tokens per frame, one-frame convs on 32x16, 16x8 and 8x4) through edm2.sampler against the oracle's
    edm_sample_frame -- guidance 1 (cached evaluations) and 1.5 (the guided pair evaluation); bounds of test_g9_sampler_rollout."""
    from edm2.networks_edm2 import UNet, Precond
    from edm2.sampler import edm_sampler_with_mse
    cfg, H, W = PORTRAIT
    p = paramgen.prenormalise(paramgen.precond_params(cfg, 303))
    net = _load(Precond(UNet(**cfg), use_fp16=True, sigma_data=0.5), p).eval()
    g = torch.Generator().manual_seed(78)
    ctx = torch.randn(1, 4, 8, H, W, generator=g) * 0.5
    lab = torch.randint(0, 4, (1, 4), generator=g)
    noise = torch.randn(1, 1, 8, H, W, generator=g)
    sig = torch.ones(1, 4) * 0.05
    cond = torch.full((1, 1), 2)
    kw = dict(num_steps=4, sigma_min=0.01, sigma_max=80, rho=2)
    with torch.no_grad():
        D, cache = net(ctx.to(DEV), sig.to(DEV), lab.to(DEV), update_cache=True)
        x, _, _, cache = edm_sampler_with_mse(net, cache, conditioning=cond.to(DEV), guidance=guidance, S_churn=0, noise=noise.to(DEV), **kw)
        R, oc = O.precond_forward(p, cfg, ctx, sig, lab, cache={}, update_cache=True, training=False, sigma_data=0.5)
        xr, oc = O.edm_sample_frame(p, cfg, oc, noise, conditioning=cond, sigma_data=0.5, guidance=guidance, **kw)
    e0, e1 = rel(D, R), rel(x, xr)
    print("portrait rollout, guidance", guidance, "prefill", e0, "generated frame", e1)
    assert cache["n_context_frames"] == oc["n_context_frames"] == 5
    assert e0 < 2e-2 and e1 < 5e-2


# ---------------------------------------------------------------------------------------------------------------------
# 5. the edge of the domain: refused, never miscomputed

def test_conv3x3_size_ok_states_the_domain():
    from autoregressive_diffusion_amd import ops
    for H in range(1, 70):
        for W in range(1, 70):
            want = (W % 16 == 0 and H % 8 == 0) or (W in (8, 4, 2) and H % W == 0)
            assert ops.conv3x3_size_ok(H, W) == want, (H, W)
    assert ops.conv3x3_size_ok(8, 4) and not ops.conv3x3_size_ok(4, 8)            # portrait / landscape asymmetry
    assert not ops.conv3x3_size_ok(12, 16) and not ops.conv3x3_size_ok(0, 16)


def _pair_bank(cin, cout):
    p2, p3 = torch.nn.Parameter(torch.randn(cout, cin, 3, 3).to(DEV)), torch.nn.Parameter(torch.randn(cout, cin, 2, 3, 3).to(DEV))
    bank, (pw2, pw3) = make_bank([p2, p3])
    bank.prepare(training=True)
    return bank, p2, p3, pw2, pw3


def _untouched(bank, pws, params, grads_before):
    torch.cuda.synchronize()
    for pw in pws:
        assert int(pw.nsplit.item()) == 0, "a split-K slab was written"
    for p, g in zip(params, grads_before):
        assert (p.grad is None) == (g is None) and (g is None or torch.equal(p.grad.view(torch.int32), g.view(torch.int32))), "a weight gradient changed"


@pytest.mark.parametrize("H,W", [(4, 8), (4, 16), (12, 8), (6, 4), (3, 2), (16, 24)])
def test_unsupported_sizes_are_refused_before_any_launch(H, W):
    """Outside ops.conv3x3_size_ok: ops.conv and ops.gated_conv_train raise OnirisError naming the size, with and without autograd,
    nothing is launched (census), and a supported launch that follows on the same stream is correct."""
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(H * 31 + W)
    cin, cout, B, T = 64, 64, 1, 2
    N = B * 2 * T
    bank, p2, p3, pw2, pw3 = _pair_bank(cin, cout)
    grads = [None if p.grad is None else p.grad.clone() for p in (p2, p3)]
    x = nhwc(torch.randn(N, cin, H, W))
    gate = (torch.rand(N) * 0.6 + 0.05).to(DEV)
    before = ops.census_peek()
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            xx = x.clone().requires_grad_(grad)
            with pytest.raises(ops.OnirisError, match=f"{H}x{W}"):
                ops.conv(xx, pw2)
            with pytest.raises(ops.OnirisError, match=f"{H}x{W}"):
                ops.gated_conv_train(xx, gate, pw2, pw3, B, T)
    after = ops.census_peek()
    assert not families({k: n - before.get(k, 0) for k, n in after.items() if n != before.get(k, 0)}), "a conv kernel was launched"
    _untouched(bank, (pw2, pw3), (p2, p3), grads)
    # the same weights on a supported size right behind it
    w = packed_weight(pw2, cout, cin, (3, 3))
    x0 = bfr(torch.randn(N, cin, 8, 16))
    with torch.no_grad():
        y = ops.conv(nhwc(x0), pw2)
    assert sd(nchw(y)[:, :cout], bfr(F.conv2d(x0.double(), w.double(), padding=1).float())) <= TIGHT


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("B,T,H,W,cout", [(2, 3, 12, 16, 32), (1, 9, 4, 16, 32), (1, 5, 12, 32, 24), (3, 2, 20, 16, 8)])
def test_streaming_forward_without_gradients_on_4_row_tiles(B, T, H, W, cout):
    """W % 16 == 0 with H % 4 == 0 and H % 8 != 0: the gated 32 -> <= 32 forward under no_grad is served by the streaming kernel (an
    odd number of 4-row tiles exists nowhere else) and matches the oracle and its bf16-faithful form."""
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(3 + H)
    cin, N = 32, B * 2 * T
    w2 = O.normalize(O.normalize(torch.randn(cout, cin, 3, 3)))
    w3 = O.normalize(O.normalize(torch.randn(cout, cin, 2, 3, 3)))
    p2, p3 = torch.nn.Parameter(w2.clone().to(DEV)), torch.nn.Parameter(w3.clone().to(DEV))
    bank, (pw2, pw3) = make_bank([p2, p3])
    bank.prepare(training=False)
    x0 = bfr(torch.randn(N, cin, H, W))
    g0 = torch.rand(N) * 0.6 + 0.05
    before = ops.census_peek()
    with torch.no_grad():
        y = ops.gated_conv_train(nhwc(x0), g0.to(DEV), pw2, pw3, B, T)
    after = ops.census_peek()
    fam = families({k: n - before.get(k, 0) for k, n in after.items() if n != before.get(k, 0)})
    assert fam == {"conv_stream_kernel<ALIAS=1>"}, fam
    assert ops._s2ctx_family(T, H, W, cin, 64, 32, T, (-2, -1), 1.0) == "stream"

    def ref(e2, e3, xin, dt):
        clean = xin.reshape(B, 2, T, cin, H, W)[:, 0]
        ctx = torch.cat([torch.ones(B, 2, cin, H, W, dtype=dt), clean], 1)
        y3 = F.conv2d(ctx[:, 0:T].reshape(B * T, cin, H, W), e3[:, :, 0], padding=1) + \
            F.conv2d(ctx[:, 1:T + 1].reshape(B * T, cin, H, W), e3[:, :, 1], padding=1)
        y3 = y3.reshape(B, 1, T, cout, H, W).expand(B, 2, T, cout, H, W).reshape(N, cout, H, W)
        return F.conv2d(xin, e2, padding=1), y3
    e2, _ = O.weight_effective(w2, 1.0, False)
    e3, _ = O.weight_effective(w3, 1.0, False)
    yr = O.mp_sum(*ref(e2, e3, x0, torch.float32), g0)
    e = rel(nchw(y)[:, :cout], yr)
    ca, cb = ops.gate_coefs(g0.to(DEV))
    y2d, y3d = ref(packed_weight(pw2, cout, cin, (3, 3)).double(), packed_weight(pw3, cout, cin, (2, 3, 3)).double(), x0.double(), torch.float64)
    faithful = bfr((ca.cpu().double().reshape(N, 1, 1, 1) * y2d + cb.cpu().double().reshape(N, 1, 1, 1) * y3d).float())
    ef = sd(nchw(y)[:, :cout], faithful)
    print("streaming forward on 4-row tiles", (B, T, H, W, cout), "rel vs oracle", e, "bf16-faithful", ef)
    assert e < 5e-3 and ef <= TIGHT
    assert_elementwise(nchw(y)[:, :cout], faithful, ("streaming forward", (B, T, H, W, cout)))


@pytest.mark.parametrize("H,W", [(12, 16), (4, 16)])
def test_forward_only_size_with_gradients_fails_before_the_forward(H, W):
    """The same shape with gradients enabled: refused in front of the forward launch, with an error that says what the weight
    gradient needs, instead of `conv_wgrad: unsupported image size` half-way through backward; no gradient buffer is touched."""
    from autoregressive_diffusion_amd import ops
    torch.manual_seed(5)
    cin, cout, B, T = 32, 32, 2, 3
    N = B * 2 * T
    bank, p2, p3, pw2, pw3 = _pair_bank(cin, cout)
    grads = [None if p.grad is None else p.grad.clone() for p in (p2, p3)]
    dwp = [pw.dwp.clone() for pw in (pw2, pw3)]
    x = nhwc(torch.randn(N, cin, H, W)).requires_grad_(True)
    gate = (torch.rand(N) * 0.6 + 0.05).to(DEV).requires_grad_(True)
    before = ops.census_peek()
    with pytest.raises(ops.OnirisError, match=r"H % 8 == 0") as info:
        ops.gated_conv_train(x, gate, pw2, pw3, B, T)
    assert f"{H}x{W}" in str(info.value) and "weight gradient" in str(info.value)
    after = ops.census_peek()
    assert not families({k: n - before.get(k, 0) for k, n in after.items() if n != before.get(k, 0)}), "the forward was launched"
    assert x.grad is None and gate.grad is None
    _untouched(bank, (pw2, pw3), (p2, p3), grads)
    # (bit patterns: the slabs are uninitialised memory until a weight-gradient launch writes them, and a NaN never equals itself)
    assert all(torch.equal(a.view(torch.int16), pw.dwp.view(torch.int16)) for a, pw in zip(dwp, (pw2, pw3))), "split-K slabs written"
    # frozen weights and no input gradient: nothing to differentiate, the forward is served
    for p in (p2, p3):
        p.requires_grad_(False)
    y = ops.gated_conv_train(x.detach(), gate.detach(), pw2, pw3, B, T)
    assert tuple(y.shape) == (N, H, W, cout) and bool(torch.isfinite(y.float()).all())
