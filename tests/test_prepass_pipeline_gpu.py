"""The backward pre-pass entry points at the shapes where a software-pipelined pixel loop can go wrong (csrc/weights.hip:
gconv_bwd_fused modes 1 and 2, whose loop requests the loads of pixel step k + AHEAD before it computes and stores step k;
gconv_bwd_prep and csrc/elementwise.hip emb_silu_bwd, which keep the plain loop and are held to the same cases), element by
element against the float64 restatements of tests/glue_oracle.py with the bounds of tests/oracle_hold.py, exactly as
tests/test_glue_stages_gpu.py uses them.  No element is left out.

Shapes.  A block's threads are npl = 256 / (C / 8) pixel lanes times C / 8 channel groups; lane pl owns the pixel steps pl,
pl + npl, ... of its slice.  The loop has a prologue (AHEAD steps requested), whole rounds of AHEAD + 1 steps, and a tail of at
most 2 AHEAD steps, so P is chosen per C such that lanes own 0, 1, 2, 3 and 4 steps, the counts on either side of every path
at AHEAD = 1 (shipped), with the ragged cases (some lanes one step short) in between; P = 2 npl + 1 and 5 npl + 7 (C = 64: 65, 167)
are the same edges for AHEAD = 2.
  C = 8    one channel group, npl = 256          C = 40   five groups (no power of two), npl = 51, one idle thread
  C = 64   npl = 32                              C = 512  64 groups, npl = 4
One slice: P < 4 npl.  Two slices, ragged in both: gconv_bwd_fused from P >= 4 npl on (the last two P of each row),
emb_silu_bwd from P >= 8 npl on (the last one).  B in {1, 2}, T in {2, 3} go round the cases; both `nt_policy` settings.
Longest chain of fp32 additions behind a reduction: 8 per pixel step, at most 5 steps, + 6 + 4 + 1 = 51 of the bound's 128.
Every figure is printed as `PREPASS <case> <tensor> <worst error / bound>` (pytest -s)."""
import pytest
import torch

import glue_oracle as GO
from oracle_hold import out as _out, hold_bf16, hold_f32, hold_exact

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
NAN = float("nan")
TAG = "PREPASS"
torch.set_num_threads(min(16, torch.get_num_threads()))


def _api():
    from autoregressive_diffusion_amd import ops
    from autoregressive_diffusion_amd._lib import lib, check
    return ops, lib, check


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rn(gen, *shape, scale=1.0, lim=8.0):
    return (torch.randn(*shape, generator=gen) * scale).clamp(-lim, lim).to(BF16)


def _g(t):
    return None if t is None else t.to(DEV).contiguous()


def _clipped_out(gen, n, clip=256.0):
    """A forward output with elements at exactly +-clip and one bf16 step inside it."""
    o = _rn(gen, n, scale=100.0, lim=clip)
    o[::7], o[1::7], o[2::7], o[3::7] = clip, -clip, clip - 1, -(clip - 1)
    return o


def _shapes():
    """(C, P) with npl = 256 / (C / 8): below one step, exactly 1, 1 | 2, 2 | 3, 3 | 4 steps per lane, then 5 npl + 7 and 8 npl + 9."""
    res = []
    for C in (8, 40, 64, 512):
        npl = 256 // (C // 8)
        for P in sorted({max(1, npl // 6), npl - 1, npl, npl + 1, 2 * npl + 1, 3 * npl + 7 if npl > 7 else 3 * npl + 3, 5 * npl + 7, 8 * npl + 9}):
            res.append((C, P))
    return res


SHAPES = _shapes()
BT = [(1, 2), (2, 3), (1, 3), (2, 2)]
CASES = [(BT[i % 4][0], BT[i % 4][1], P, C) for i, (C, P) in enumerate(SHAPES)]


def test_shapes_cover_every_path_of_the_loop():
    """The step counts the module docstring promises, per C: a lane with no step, and lanes with 1 .. 4 steps in one slice."""
    for C in (8, 40, 64, 512):
        npl, seen = 256 // (C // 8), set()
        for c, P in SHAPES:
            if c == C and P < 4 * npl:
                seen |= {len(range(pl, P, npl)) for pl in range(npl)}
        assert {0, 1, 2, 3, 4} <= seen, (C, seen)
        assert any(c == C and P >= 4 * npl and (P + 1) // 2 % npl for c, P in SHAPES), C


def _gate_inputs(gen, B, T, P, C):
    return (_rn(gen, B, 2, T, P, C), _rn(gen, B, 2, T, P, C, scale=2.0, lim=5.0), _rn(gen, B, T, P, C),
            torch.rand(B, 2, T, generator=gen) * 0.5 + 0.5, torch.rand(B, 2, T, generator=gen) - 0.5)


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("B,T,P,C", CASES)
def test_gconv_bwd_fused_mode1(B, T, P, C, padded):
    """cscale_pitch = 0 (rows of C) and C + 8 with NaN in the padding."""
    ops, lib, check = _api()
    gen = _gen(11000 + 7 * C + P)
    pitch = C + 8 if padded else 0
    case = f"fused1({B},{T},{P},{C},pitch={pitch})"
    g, raw, y3, ca, cb = _gate_inputs(gen, B, T, P, C)
    cs = torch.rand(B, 2, T, C, generator=gen) + 0.5
    csfull = torch.full((B, 2, T, pitch or C), NAN)
    csfull[..., :C] = cs
    dout, dy3 = _out(B, 2, T, P, C), _out(B, T, P, C)
    dca, dcb, dcs = (_out(B, 2, T, dtype=torch.float32, fill=0.0), _out(B, 2, T, dtype=torch.float32, fill=0.0),
                     _out(B, 2, T, C, dtype=torch.float32, fill=0.0))
    dev = [_g(t) for t in (g, raw, y3, ca, cb, csfull)]
    check(lib.oniris_gconv_bwd_fused(1, *[ops._p(t) for t in dev], None, ops._p(dout), None, ops._p(dy3), ops._p(dca), ops._p(dcb),
                                     ops._p(dcs), B, T, P, C, 1.0, 1.0, 0.0, pitch, None, None, ops._stream()), "gconv_bwd_fused")
    torch.cuda.synchronize()
    rdout, _, rdy3, rca, rcb, rcs, _ = GO.gconv_fused(1, g, raw, y3, ca, cb, cs, None, 1.0, 1.0, 0.0, False, 0, dout_bf16=dout)
    hold_bf16(case, "dout", dout, rdout, TAG)
    hold_bf16(case, "dy3", dy3, rdy3, TAG)
    hold_f32(case, "dca", dca, rca, TAG)
    hold_f32(case, "dcb", dcb, rcb, TAG)
    hold_f32(case, "dcs", dcs, rcs, TAG)


MODE2_VARIANTS = ["plain", "clip", "alias-flag0", "alias-flag1", "alias-noclip", "alias-flag1-nodres"]


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("variant", MODE2_VARIANTS)
@pytest.mark.parametrize("B,T,P,C", CASES)
def test_gconv_bwd_fused_mode2(B, T, P, C, variant):
    """Not alias with clip 0 / 256; alias with the flag clear and xo full of values >= clip (g must come back untouched), with the
    flag set (g masked IN PLACE -- the loads requested ahead must not see a rewritten element, nor a store hit an element whose
    load is still due: g' equals the oracle's masked g exactly, ragged tails included -- with dres given and NULL), and with
    clip <= 0 and no flag.  xo holds elements at exactly +-256 and +-255."""
    ops, lib, check = _api()
    gen = _gen(12000 + 7 * C + P)
    case = f"fused2({B},{T},{P},{C}) {variant}"
    alias = "alias" in variant
    clip = 0.0 if variant in ("plain", "alias-noclip") else 256.0
    flag = None if (not alias or clip <= 0) else (0 if variant == "alias-flag0" else 1)
    with_dres = variant != "alias-flag1-nodres"
    ta, tb = 0.8, 0.6
    g, raw, y3, ca, cb = _gate_inputs(gen, B, T, P, C)
    if variant == "alias-flag0":
        xo = torch.full((B, 2, T, P, C), 300.0).to(BF16)
    else:
        xo = _clipped_out(gen, B * 2 * T * P * C).reshape(B, 2, T, P, C)
    gg = _g(g).clone()
    dout = gg if alias else _out(B, 2, T, P, C)
    dres, dy3 = (_out(B, 2, T, P, C) if with_dres else None), _out(B, T, P, C)
    dca, dcb = _out(B, 2, T, dtype=torch.float32, fill=0.0), _out(B, 2, T, dtype=torch.float32, fill=0.0)
    cas = _out(B, 2, T, dtype=torch.float32) if alias else None
    fl = torch.tensor([flag], dtype=torch.int32, device=DEV) if flag is not None else None
    dev = [_g(t) for t in (raw, y3, ca, cb)]
    xog = _g(xo)
    check(lib.oniris_gconv_bwd_fused(2, ops._p(gg), *[ops._p(t) for t in dev], None, ops._p(xog) if clip > 0 else None, ops._p(dout),
                                     ops._p(dres), ops._p(dy3), ops._p(dca), ops._p(dcb), None, B, T, P, C, ta, tb, clip, 0, ops._p(fl),
                                     ops._p(cas), ops._stream()), "gconv_bwd_fused")
    torch.cuda.synchronize()
    rfirst, rres, rdy3, rca, rcb, _, rcas = GO.gconv_fused(2, g, raw, y3, ca, cb, None, xo, ta, tb, clip, alias, flag or 0,
                                                           dout_bf16=None if alias else dout)
    if alias:
        hold_exact(case, "g'", gg, rfirst[0], TAG)             # masking is exact: g itself, or g with zeros
        if variant == "alias-flag0":
            assert torch.equal(gg.cpu(), g), "flag = 0: g must come back untouched"
        if flag == 1:
            assert int((gg.cpu() != g).sum()) > 0, "flag = 1: the probe must mask something"
        hold_f32(case, "ca_scaled", cas, rcas, TAG)
    else:
        hold_bf16(case, "dout", dout, rfirst, TAG)
    if with_dres:
        hold_bf16(case, "dres", dres, rres, TAG)
    hold_bf16(case, "dy3", dy3, rdy3, TAG)
    hold_f32(case, "dca", dca, rca, TAG)
    hold_f32(case, "dcb", dcb, rcb, TAG)


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("B,T,P,C", CASES)
def test_emb_silu_bwd(B, T, P, C, padded):
    """N = B * T frames; c_pitch = 0 and C + 8 with NaN in the padding."""
    ops, lib, check = _api()
    gen = _gen(13000 + 7 * C + P)
    N, pitch = B * T, (C + 8 if padded else 0)
    case = f"emb_silu_bwd({N},{P},{C},pitch={pitch})"
    du, y = _rn(gen, N, P, C), _rn(gen, N, P, C, scale=2.0, lim=5.0)
    c = torch.rand(N, C, generator=gen) + 0.5
    cfull = torch.full((N, pitch or C), NAN)
    cfull[:, :C] = c
    dy, dc = _out(N, P, C), _out(N, C, dtype=torch.float32, fill=0.0)
    dug, yg, cg = _g(du), _g(y), _g(cfull)
    check(lib.oniris_emb_silu_bwd(ops._p(dug), ops._p(yg), ops._p(cg), ops._p(dy), ops._p(dc), N, P, C, pitch, 1, ops._stream()),
          "emb_silu_bwd")
    torch.cuda.synchronize()
    rdy, rdc = GO.emb_silu_bwd(du, y, c)
    hold_bf16(case, "dy", dy, rdy, TAG)
    hold_f32(case, "dc", dc, rdc, TAG)


# one step of gconv_bwd_prep is 256 lanes x 8 elements: below one step, 1, 1 | 2, 3 | 4 steps; two slices from 8192 elements on
PREP_FE = [40, 2040, 2048, 2056, 6200, 8200, 14344]


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("i,fe", list(enumerate(PREP_FE)))
def test_gconv_bwd_prep(i, fe, S):
    ops, lib, check = _api()
    B, T = BT[i % 4]
    gen = _gen(14000 + fe)
    case = f"gconv_bwd_prep({B},{S},{T},{fe})"
    dout, o, y3 = _rn(gen, B, S, T, fe), _rn(gen, B, S, T, fe), _rn(gen, B, T, fe)
    ca, cb = torch.rand(B, S, T, generator=gen) * 0.5 + 0.5, torch.rand(B, S, T, generator=gen) - 0.5
    dca, dcb = _out(B, S, T, dtype=torch.float32, fill=0.0), _out(B, S, T, dtype=torch.float32, fill=0.0)
    dy3 = _out(B, T, fe)
    dev = [_g(t) for t in (dout, o, y3, ca, cb)]
    check(lib.oniris_gconv_bwd_prep(*[ops._p(t) for t in dev], ops._p(dca), ops._p(dcb), ops._p(dy3), B, S, T, fe, ops._stream()),
          "gconv_bwd_prep")
    torch.cuda.synchronize()
    rca, rcb, ry3 = GO.gconv_prep(dout, o, y3, ca, cb, S)
    hold_f32(case, "dca", dca, rca, TAG)
    hold_f32(case, "dcb", dcb, rcb, TAG)
    hold_bf16(case, "dy3", dy3, ry3, TAG)
