"""The weight and optimizer kernels (upper half of csrc/weights.hip: weight_prep_kernel, weight_wb_kernel, weight_bwd_kernel,
adamw_kernel, sqnorm_partial_kernel / sqnorm_final_kernel) element by element against their float64 restatements
(tests/weight_oracle.py, reviewed by tests/test_weight_oracle.py).  One launch against one restatement fed with exactly what the
kernel read; every tensor at every element; every figure printed as `WEIGHT <case> <tensor> <worst error / bound>` (pytest -s,
profiles/weight_stage_tests.txt).

Bounds (derived in tests/weight_oracle.py, with the chain lengths per weight):
  wf, wb                       2^-8 |ref| + 2^-18 mag
  w_new, p, m, v, EMA copies   2^-18 mag
  grad, sqnorm on Gaussians    2^-17 mag
  exact                        padding of wf / wb (bit-zero), wb against the transpose of the kernel's own wf, eval parameters,
                               identity rows, .grad at nsplit = 0 and after a second backward(), p / m / v at step 0, g, every
                               guard element, sqnorm on ternary data

One bank carries all the weights, so that row_start / tile_start are irregular prefix sums and every descriptor lookup of the
three kernels crosses descriptor borders:
   #  rows  tiles  weight
   1    24      1  (24, 16), gain 0.8                   linear, fewer than 32 rows
   2    40      2  (40, 24, 1, 1)                       second tile of 8 rows; row 3 all zero, row 17 scaled by 1e-12
   3    13      1  (13, 8, 3, 3)                        cout % 8 != 0: the scalar tail of weight_wb
   4     8      1  (8, 5, 3, 3)                         cin & 7 != 0: the fallback pack and the four-chain weight_bwd
   5    16      1  (16, 288, 2, 3, 3)                   18 taps, LDS rounds of 256 + 32 channels, flip within the temporal slice
   6     8      1  (8, 640, 3, 3)                       9 taps, rounds of 512 + 128
   7   192      6  (192, 64, 1, 1), perm3               qkv rows (m c s) -> (s m c) in wf, wb and the slabs
   8    32      1  (32, 160, 3, 3), need_dgrad=False    wb == NULL
   9  64 + 96 + 40  (64, 64), (96, 64), (40, 64) joined by add_group: member rows 0, 64, 192 of 256, one shared nsplit
  10    32      1  (32, 32, 3, 3), requires_grad=False  packed, never given a gradient (grad == NULL)"""
import functools
import math

import pytest
import torch

import oracle_hold as OH
import weight_oracle as WO

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
F32 = torch.float32
GUARD = 64
MARK = 777.0
torch.set_num_threads(min(16, torch.get_num_threads()))

hold_bf16 = functools.partial(OH.hold_bf16, tag="WEIGHT")
hold_f32 = functools.partial(OH.hold_f32, tag="WEIGHT")
hold_f32_elem = functools.partial(OH.hold_f32_elem, tag="WEIGHT")
hold_exact = functools.partial(OH.hold_exact, tag="WEIGHT")

SPECS = [  # name, shape, add() arguments, group member, trainable
    ("w1", (24, 16), dict(gain=0.8), False, True),
    ("w2", (40, 24, 1, 1), {}, False, True),
    ("w3", (13, 8, 3, 3), {}, False, True),
    ("w4", (8, 5, 3, 3), {}, False, True),
    ("w5", (16, 288, 2, 3, 3), {}, False, True),
    ("w6", (8, 640, 3, 3), {}, False, True),
    ("w7", (192, 64, 1, 1), dict(perm3=True), False, True),
    ("w8", (32, 160, 3, 3), dict(need_dgrad=False), False, True),
    ("g0", (64, 64), {}, True, True),
    ("g1", (96, 64), {}, True, True),
    ("g2", (40, 64), {}, True, True),
    ("w10", (32, 32, 3, 3), {}, False, False),
]
GOFF = {"g0": 0, "g1": 64, "g2": 192}
CTOT = 256


def _ops():
    from autoregressive_diffusion_amd import ops
    return ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _kt(shape):
    return shape[2] if len(shape) == 5 else 1


def _taps(shape):
    return math.prod(shape[2:]) if len(shape) > 2 else 1


@functools.lru_cache(maxsize=None)
def _weights():
    gen = _gen(11)
    ws = [torch.randn(*shape, generator=gen) * 1.7 for _, shape, _, _, _ in SPECS]
    ws[1][3] = 0.0                                        # finite everywhere, equal to the restatement: s = eps, k2 = 0
    ws[1][17] *= 1e-12
    return ws


@functools.lru_cache(maxsize=None)
def _grads0():
    gen = _gen(12)
    return [torch.randn(*shape, generator=gen) + 3.0 for _, shape, _, _, _ in SPECS]


def _bank(with_grads=False):
    ops = _ops()
    bank = ops.WeightBank()
    params, pws = [], []
    for (name, shape, kw, _, trainable), w, g0 in zip(SPECS, _weights(), _grads0()):
        p = torch.nn.Parameter(w.clone().to(DEV), requires_grad=trainable)
        if with_grads and trainable:
            p.grad = g0.clone().to(DEV)
        params.append(p)
        pws.append(bank.add(p, **kw))
    group = bank.add_group([pw for pw, s in zip(pws, SPECS) if s[3]])
    assert [pw.goff for pw, s in zip(pws, SPECS) if s[3]] == [0, 64, 192] and group.cout == CTOT
    return bank, params, pws, group


def _ref_args(i):
    name, shape, kw, member, _ = SPECS[i]
    a = dict(perm3=kw.get("perm3", False), eps=WO.EPS_F32)
    if member:
        a["goff"] = GOFF[name]
    return WO.f32(kw.get("gain", 1.0)), a


@functools.lru_cache(maxsize=None)
def _prep_ref(i, training):
    name, shape, kw, member, _ = SPECS[i]
    gain, a = _ref_args(i)
    return WO.prep(_weights()[i], gain, training, kt=_kt(shape), rows=CTOT if member else None, **a)


def _bits(t):
    return t.detach().cpu().view(torch.int16)


def _hold_image(case, name, got, pair, live):
    """A whole padded bf16 image: the bf16 bound on every element, and the padding bit-zero (not -0)."""
    hold_bf16(case, name, got, pair)
    pad = _bits(got).reshape(live.shape)[~live]
    assert bool((pad == 0).all()), f"{case} {name}: {int((pad != 0).sum())} padding elements are not bit-zero"


# ---------------------------------------------------------------------------------------------------------------------
# weight_prep_kernel + weight_wb_kernel
@pytest.mark.parametrize("training", [True, False])
def test_prep_one_bank_many_descriptors(training):
    """prepare(training) on a fresh bank: the written-back parameters (eval: the input bits), the whole padded wf and wb images of
    every weight and of the group's matrices, nsplit reset."""
    bank, params, pws, group = _bank()
    bank._ensure()                                        # (the table and the nsplit slots exist before the launch under test)
    bank.nsplit_all.fill_(5)
    bank.prepare(training)
    torch.cuda.synchronize()
    mode = "train" if training else "eval"
    assert (bank.total_rows, bank.total_tiles) == (24 + 40 + 13 + 8 + 16 + 8 + 192 + 32 + 200 + 32, 1 + 2 + 1 + 1 + 1 + 1 + 6 + 1 + 2 + 3 + 2 + 1)
    gsum = None
    for i, (name, shape, kw, member, _) in enumerate(SPECS):
        case, r, pw = f"prep[{mode}] {name}{shape}", _prep_ref(i, training), pws[i]
        assert not bool(r.identity.any())
        if training:
            hold_f32_elem(case, "w_new", params[i].data, r.w_new)
        else:
            hold_exact(case, "w", params[i].data, _weights()[i])
        assert int(pw.nsplit.item()) == 0, f"{case}: nsplit not reset"
        if member:
            parts = (r.wf[0], r.wf[1], r.wf_live, r.wb[0], r.wb[1], r.wb_live)
            gsum = parts if gsum is None else tuple(a | b if a.dtype == torch.bool else a + b for a, b in zip(gsum, parts))
            continue
        taps = _taps(shape)
        wf = pw.wf.view(taps, pw.CoutP, pw.CinP)
        _hold_image(case, "wf", wf, r.wf, r.wf_live)
        if kw.get("need_dgrad", True):
            wb = pw.wb.view(taps, pw.CoutPb, pw.CinPb)
            _hold_image(case, "wb", wb, r.wb, r.wb_live)
            hold_exact(case, "wb == wf^T", wb.float(), WO.wb_of(wf.cpu(), shape[0], shape[1], _kt(shape), pw.CoutPb, pw.CinPb).float())
        else:
            assert pw.wb is None
    case = f"prep[{mode}] group(64+96+40, 64)"
    wf, wb = group.wf.view(1, CTOT, 64), group.wb.view(1, 64, CTOT)
    _hold_image(case, "wf", wf, gsum[0:2], gsum[2])
    _hold_image(case, "wb", wb, gsum[3:5], gsum[5])
    want = sum(WO.wb_of(wf.cpu(), SPECS[i][1][0], 64, 1, 64, CTOT, goff=GOFF[SPECS[i][0]]).float() for i in (8, 9, 10))
    hold_exact(case, "wb == wf^T", wb.float(), want)
    assert int(group.nsplit.item()) == 0


# the identity rule: |den - 1| < 4e-7 in fp32 leaves the row as it is
IDENT_INSIDE = 5e-8        # rows used as "inside":  float64 |den - 1| <= 5e-8
IDENT_OUTSIDE = 2e-6       # rows used as "outside": float64 |den - 1| >= 2e-6
IDENT_EMULATED = 2.4e-7    # ... and, for the inside rows, the float32 evaluation in the kernel's order within 2 ulp of 1 as well


@functools.lru_cache(maxsize=None)
def _identity_rows():
    """A (12, 256) weight (fan = 256: one element per thread, sqrt(fan) exact): even rows inside, odd rows outside.
    The kernel's fp32 den differs from the float64 one by the roundoffs of the sum (one per product, 6 butterfly steps, 3 additions
    of the waves' sums: 10 u, halved by the square root), of sqrt, of the product with 1/16 (exact) and of the addition of eps:
    7 u = 4.2e-7 if every roundoff pointed the same way, about a third of that as a root of the sum of squares.  (The issue's
    "about 3.2e-7" counts 9 roundoffs on the sum and nothing for the products; the worst case is larger, as stated here.)  An inside
    row (<= 5e-8) is therefore certain to stay below 4e-7 only up to 3.5e-7 of fp32 error, i.e. short of the strict worst case
    by 0.7e-7: the search also asks the float32 evaluation in the kernel's order to land within 2.4e-7, which costs no row.
    Outside rows (>= 2e-6) are five times the threshold away.  No row between the margins is used."""
    gen = _gen(13)
    fan, rows = 256, []
    offsets = [2.5e-6, -2.5e-6, 4e-6, -4e-6, 1e-5, -2.1e-6]
    while len(rows) < 12:
        r = torch.randn(fan, generator=gen, dtype=torch.float64)
        outside = len(rows) % 2 == 1
        off = offsets[len(rows) // 2] if outside else 0.0
        row = (r * ((1 + off - WO.EPS_F32) * 16.0 / r.norm())).float()
        d64 = abs(float(WO.row_den(row[None], WO.EPS_F32)[0]) - 1)
        d32 = abs(float(WO.row_den(row[None], WO.EPS_F32, torch.float32)[0]) - 1)
        if (outside and d64 >= IDENT_OUTSIDE) or (not outside and d64 <= IDENT_INSIDE and d32 <= IDENT_EMULATED):
            rows.append(row)
    return torch.stack(rows)


def test_identity_rule():
    w = _identity_rows()
    d64 = (WO.row_den(w, WO.EPS_F32) - 1).abs()
    inside = torch.arange(12) % 2 == 0
    assert bool((d64[inside] <= IDENT_INSIDE).all()) and bool((d64[~inside] >= IDENT_OUTSIDE).all())
    print(f"identity rows: float64 |den - 1| inside <= {d64[inside].max():.2e}, outside >= {d64[~inside].min():.2e}")
    ops = _ops()
    bank = ops.WeightBank()
    p = torch.nn.Parameter(w.clone().to(DEV))
    pw = bank.add(p)
    bank.prepare(training=True)
    torch.cuda.synchronize()
    r = WO.prep(w, 1.0, True, eps=WO.EPS_F32)
    assert torch.equal(r.identity, inside)
    got = p.data.cpu()
    hold_exact("identity", "rows inside", got[inside], w[inside])
    hold_f32_elem("identity", "rows outside", got[~inside], (r.w_new[0][~inside], r.w_new[1][~inside]))
    assert bool((got[~inside] != w[~inside]).any(dim=1).all()), "an outside row came back with its input bits"
    hold_bf16("identity", "wf", pw.wf.view(1, pw.CoutP, pw.CinP), r.wf)


# ---------------------------------------------------------------------------------------------------------------------
# weight_bwd_kernel
#            w1  w2  w3  w4  w5  w6  w7  w8  group  w10       transposing form: {0, 1, 2, 7, 8, 9, 19}; w4 (four chains): {1, 3, 4, 5, 9}
NSPLIT = {"A": (7, 2, 1, 3, 19, 9, 8, 0, 9, 2),
          "B": (0, 8, 19, 5, 1, 7, 2, 9, 1, 1),
          "C": (9, 19, 8, 9, 2, 0, 1, 7, 8, 1),
          "D": (1, 1, 2, 1, 8, 8, 19, 19, 0, 1),
          "E": (2, 7, 9, 4, 7, 19, 9, 2, 19, 1),
          "gauss": (19, 19, 19, 9, 19, 19, 19, 19, 19, 1)}


def _count(assign, i):
    return NSPLIT[assign][min(i, 8) if i < 11 else 9]


def _fill_slabs(gen, ns, rows, taps, cin, live_rows, integers):
    """(ns + 1, rows, taps, CinP) bf16: NaN in every padded row and column and in the whole slab behind the last valid one."""
    CinP = WO.roundup(cin, 64)
    s = torch.full((ns + 1, rows, taps, CinP), float("nan"), dtype=BF16)
    for lo, hi in live_rows:
        shape = (ns, hi - lo, taps, cin)
        s[:ns, lo:hi, :, :cin] = (torch.randint(-4, 5, shape, generator=gen).float() if integers else torch.randn(*shape, generator=gen)).to(BF16)
    return s


@pytest.mark.parametrize("assign", list(NSPLIT))
def test_bwd_one_bank_many_descriptors(assign):
    """Slabs filled by hand, per descriptor its own slab count, .grad pre-filled: every gradient element against `bwd`.  Integer slabs
    in [-4, 4] (G exact: a misplaced, lost or doubled entry shows at full size) or, once, Gaussian bf16 slabs at 19."""
    bank, params, pws, group = _bank(with_grads=True)
    bank.prepare(training=True)
    torch.cuda.synchronize()
    gen = _gen(100 + len(assign) + ord(assign[0]))
    integers = assign != "gauss"
    w_read = [p.data.cpu().clone() for p in params]
    slabs = {}
    for i, (name, shape, kw, member, trainable) in enumerate(SPECS):
        if member:
            continue
        ns, pw = _count(assign, i), pws[i]
        assert ns + 1 <= pw.nsplit_cap
        s = slabs[name] = _fill_slabs(gen, ns, pw.CoutP, _taps(shape), shape[1], [(0, shape[0])], integers)
        pw.dwp[:s.numel()].copy_(s.reshape(-1))
        pw.nsplit.fill_(ns)
    ns = _count(assign, 8)
    sg = _fill_slabs(gen, ns, CTOT, 1, 64, [(GOFF[n], GOFF[n] + SPECS[i][1][0]) for i, n in ((8, "g0"), (9, "g1"), (10, "g2"))], integers)
    group.dwp[:sg.numel()].copy_(sg.reshape(-1))
    group.nsplit.fill_(ns)
    assert all(pws[i].nsplit.data_ptr() == group.nsplit.data_ptr() for i in (8, 9, 10))
    bank.backward()
    torch.cuda.synchronize()
    first = []
    for i, (name, shape, kw, member, trainable) in enumerate(SPECS):
        ns = _count(assign, i)
        case = f"bwd[{assign}] {name}{shape} nsplit={ns}"
        hold_exact(case, "w untouched", params[i].data, w_read[i])
        if not trainable:
            assert params[i].grad is None
            first.append(None)
            continue
        first.append(params[i].grad.clone())
        gain, a = _ref_args(i)
        if ns == 0:
            hold_exact(case, "grad untouched", params[i].grad, _grads0()[i])
            continue
        hold_f32(case, "grad", params[i].grad, WO.bwd(w_read[i], sg if member else slabs[name], ns, gain, _grads0()[i], **a))
    assert int(bank.nsplit_all.abs().sum().item()) == 0, "backward() leaves nsplit_all zero"
    bank.backward()                                       # the slabs are consumed: nothing may change
    torch.cuda.synchronize()
    for i, g1 in enumerate(first):
        if g1 is not None:
            assert torch.equal(params[i].grad, g1), f"bwd[{assign}] {SPECS[i][0]}: a second backward() changed .grad"
    print(f"WEIGHT bwd[{assign}] second backward() exact")


# ---------------------------------------------------------------------------------------------------------------------
# adamw_kernel
HYPER = (1e-2, 0.9, 0.99, 1e-8, 0.01)
LOUD = (0.05, 0.8, 0.95, 1e-6, 0.1)                       # (lr * wd and 1 - beta large enough that their ORDER shows)
BIG = 4194304 + 4099       # 4096 blocks * 256 threads * 4: the first 1024 threads take a second trip, thread 1024 a 3-element tail behind it
LO = 4
ADAMW = [  # n, step, clip (None / "active" / "inactive"), EMA copies, grad_scale, norm_ready, hyper
    (1, 1, None, 0, 1.0, False, HYPER),                   # oniris_adamw, the tail alone
    (3, 0, None, 2, 1.0, False, HYPER),                   # step 0: EMA only
    (4, 3, "active", 1, 0.5, False, HYPER),
    (5, 1000, "inactive", 2, 1.0 / 1024, False, HYPER),
    (1023, 3, "active", 2, 1.0, True, HYPER),
    (4097, 1, "inactive", 0, 0.5, True, HYPER),
    (4097, 0, "active", 1, 0.5, True, HYPER),             # step 0 with a clip requested: the norm is not read
    (1023, 1000, None, 1, 1.0, False, LOUD),
    (5, 3, "inactive", 0, 1.0, False, LOUD),
    (4, 0, None, 0, 1.0, False, HYPER),                   # step 0 without EMA copies: nothing to do
    (BIG, 3, "active", 2, 0.5, True, HYPER),
    (BIG, 0, None, 2, 1.0, False, HYPER),
    (BIG, 1, None, 0, 1.0 / 1024, False, LOUD),
]


class Slice:
    """A read-write buffer as the product passes it: the range [LO, LO + n) of a larger one whose other elements (LO in front, 64
    behind) are guards that must come back untouched."""

    def __init__(self, values):
        self.n = values.numel()
        self.flat = torch.full((LO + self.n + GUARD,), MARK, dtype=F32, device=DEV)
        self.t = self.flat[LO:LO + self.n]
        self.t.copy_(values)

    def guards_ok(self, case, name):
        ok = bool((self.flat[:LO] == MARK).all()) and bool((self.flat[LO + self.n:] == MARK).all())
        assert ok, f"{case} {name}: the guard elements around the buffer were written"


@pytest.mark.parametrize("n,step,clip,nema,gscale,norm_ready,hyper", ADAMW)
def test_adamw(n, step, clip, nema, gscale, norm_ready, hyper):
    ops = _ops()
    gen = _gen(n + step)
    case = f"adamw[n={n},step={step},clip={clip},ema={nema},gs={gscale:g},ready={int(norm_ready)},lr={hyper[0]}]"
    p0, m0, v0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.01, torch.rand(n, generator=gen) * 1e-4
    gbig0 = torch.randn(LO + n + GUARD, generator=gen) * 0.01        # (the whole gradient buffer: with norm_ready its norm is the clip's)
    e0 = [torch.randn(n, generator=gen) for _ in range(nema)]
    ws = [0.13, 0.06][:nema]
    p, m, v, e = Slice(p0), Slice(m0), Slice(v0), [Slice(t) for t in e0]
    gbig = gbig0.to(DEV)
    g = gbig[LO:LO + n]
    normed = gbig0 if norm_ready else gbig0[LO:LO + n]
    norm = math.sqrt(float((normed.double() ** 2).sum())) * abs(gscale)
    max_norm = None if clip is None else (0.5 if clip == "active" else 2.0) * norm          # coef = 0.5 / 2: away from 1
    buf = Slice(torch.full((1 + ops.SQNORM_WS,), float("nan")))
    if norm_ready:
        ops.sqnorm_(gbig, buf.t)
    ops.adamw_(p.t, g, m.t, v.t, *hyper, step, gscale, max_norm, buf.t if clip else None, list(zip([x.t for x in e], ws)), norm_ready=norm_ready)
    torch.cuda.synchronize()
    gn = None
    if clip and step >= 1:
        gn = float(buf.t[0])                              # the value the kernel read
        hold_f32(case, "sum g^2", buf.t[:1], tuple(t.reshape(1) for t in WO.sqnorm(normed)))
    rp, rm, rv, re = WO.adamw(p0, g, m0, v0, tuple(WO.f32(x) for x in hyper), step, WO.f32(gscale), gn,
                              None if max_norm is None else WO.f32(max_norm), [(t, WO.f32(w)) for t, w in zip(e0, ws)], WO.CLIP_EPS_F32)
    if step == 0:
        for name, got, was in (("p", p, p0), ("m", m, m0), ("v", v, v0)):
            hold_exact(case, f"{name} untouched", got.t, was)
    else:
        hold_f32_elem(case, "p", p.t, rp)
        hold_f32_elem(case, "m", m.t, rm)
        hold_f32_elem(case, "v", v.t, rv)
    for k in range(nema):
        hold_f32_elem(case, f"ema{k}", e[k].t, re[k])
    hold_exact(case, "g unchanged", gbig, gbig0)
    for name, s in [("p", p), ("m", m), ("v", v), ("norm_buf", buf)] + [(f"ema{k}", x) for k, x in enumerate(e)]:
        s.guards_ok(case, name)


# ---------------------------------------------------------------------------------------------------------------------
# sqnorm_partial_kernel + sqnorm_final_kernel
@pytest.mark.parametrize("n", [1, 3, 5, 1024, 2 * 1048576 + 1203])     # the last: 1024 blocks, second and third trips, a 3-element tail
def test_sqnorm(n):
    ops = _ops()
    gen = _gen(n)
    ternary = torch.randint(-1, 3, (n,), generator=gen).clamp(max=1).float()        # -1, 0, 1, 1: three of four elements count
    signs = torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1                # every element counts
    gauss = torch.randn(n, generator=gen) * 0.01
    for kind, x in (("ternary", ternary), ("signs", signs), ("gauss", gauss)):
        case = f"sqnorm[n={n}] {kind}"
        src = Slice(x)
        outs = []
        for _ in range(2):
            buf = Slice(torch.full((1 + ops.SQNORM_WS,), float("nan")))
            ops.sqnorm_(src.t, buf.t)
            torch.cuda.synchronize()
            buf.guards_ok(case, "norm_buf")
            outs.append(buf.t[:1].clone())
        if kind == "gauss":
            hold_f32(case, "sum", outs[0], tuple(t.reshape(1) for t in WO.sqnorm(x)))
        else:
            count = float((x != 0).sum())
            assert count < 2 ** 24
            hold_exact(case, "count", outs[0], torch.tensor([count]))
        assert torch.equal(outs[0], outs[1]), f"{case}: two runs differ"
        hold_exact(case, "g unchanged", src.flat[LO:LO + n], x)
        src.guards_ok(case, "g")
