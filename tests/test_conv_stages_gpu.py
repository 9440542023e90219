"""The UNet conv kernels -- forward, data gradient, weight gradient -- element by element against their float64 restatements
(tests/conv_oracle.py, reviewed by tests/test_conv_oracle.py).  ops._conv_launch and lib.oniris_conv_wgrad_group are called directly,
one launch against one restatement fed exactly the buffers the kernel read: hand-made packed weights [taps][CoutP][CinP] whose
padded ROWS hold live values (no result may depend on them), NaN-prefilled outputs, zeroed slabs.  Every case
  (a) holds random bf16 inputs (|v| <= 8) to the derived bound, no element left out,
  (b) holds an integer-exact probe bit for bit (sparse ternary inputs times small integers, weights / coefficients / ta / tb / scale
      signed powers of two in {1, 2, 4}: test_conv_oracle.py asserts mag <= 256 for every case, which makes every partial sum in any
      order and any split an integer below 2^8, exact in fp32, in a bf16 slab and in a bf16 output),
  (c) asserts from the dispatch census that the kernel family it was aimed at is the one that ran.
Kernels launched with the `nt-stores` tag run under both `nt_policy` settings.

Bounds (conv_oracle's docstring derives them):
  bf16 outputs   2^-8 |ref| + u mag,  u = (K + 12 + 16) * 2^-24:  K = taps * Cin * (3 with the context path, else 1) products behind
                 one accumulator, 12 = the most slices the split-K path adds (it is lent its workspace in every launch of at most
                 16384 positions and takes it for the few-tile staged / one-frame launches), 16 = the epilogue's operations.
                 K per case:  Cin 24: 648 (216 plain);  Cin 32: 864 (288 plain);  Cin 40: 1080;  Cin 64: 1728 (576 plain);  1x1: Cin.
                 The evaluation-path rows add Cin 16: 432 (pair_fallback); their own-taps-only frames -- every frame of a
                 ctx_prod_mode 2 launch, the 2-D rows of a guided pair -- have K = 9 Cin: 144 / 288 / 576 / 864 / 1440 for Cin 16 /
                 32 / 64 / 96 / 160 (no bf16 output has the full chain of Cin 96 or 160 behind it: those rows are mode 2, or mode 3
                 with the fp32 product alone); the two-source 1x1 rows K = C1 + C2 = 40 / 64 / 512.
                 The longest, K = 1728, gives u = 1756 * 2^-24 = 1.05e-4 -- still 37 times below the 2^-8 of the bf16 store.
  fp32 ctx_prod  (18 Cin + 4) * 2^-24 mag: the kept context product of the one-frame kernel, 18 Cin exact products in fp32 + the four
                 partial tiles; no 2^-8 term, the store is fp32.  Exact in the probe.
  act_out        2^-8 |a| + 2^-18 |a| (glue_oracle.bound_bf16), a = silu(xo) / 0.596 of the exact two-source input xo
  activation     out2 of EPI_EMB_SILU: 2^-8 |a| + 2^-18 (1 + |z|) |a| + 2^-112, from the kernel's own bf16 `out` (z = out * escale; the
                 constant is the fp32 underflow of sigmoid(z) below z = -87, which the probes reach)
  slab sums      (2^-8 [+ 2^-8 with scale] + chain * 2^-24) mag,  chain = ceil(positions / nsplit_out) + 128 = the positions one slab
                 sums, printed per group: 176 ... 320 where every position tile has a column of its own, 512 ... 1664 for the
                 capped launches (ws_ph8, ws_out) and 2688 for wg_many (10240 positions in 4 slabs), i.e. u <= 1.6e-4.
No chain is longer than its bound assumes: K and `chain` are worst cases over every kernel family -- a kernel that deals K to waves
or slices, or positions to more slabs, only shortens them.  The bf16 outputs use 0.72 ... 0.995 of their bound -- the 2^-8 |ref| of
the one bf16 store is sharp, the same figures as the fp32 evaluation of test_conv_oracle.py -- and the slab sums 0.02 ... 0.35.

The launch forms of the evaluation path are rows of the same table: the prefill / several-frame append (S = 1 with a context and
T > 1, and the one-frame launches the streaming kernel refuses), ctx_prod_mode 1 / 2 / 3 of the one-frame kernel (mode 2 reads a
product the TEST makes, with ctx and w_ctx full of NaN), the guided pair (ctx_rows: everything the 2-D rows must not index by their
own row number has a NaN tail) with its two-launch fall-back through ops.gated_conv_eval, and the two-source 1x1 conv (x2 / act_out).

Out of scope: EPI_ACT_BWD (tests/test_skip_act_bwd_gpu.py holds it bit-identical to the two-launch form), ctx_out of the one-frame
kernel, and variants only a diagnostic big_tile bit or an environment knob can reach.
Every figure is printed as `CONV <case> <tensor> <worst error / bound>` (pytest -s); profiles/conv_stage_tests.txt has them."""
import re

import pytest
import torch

import conv_oracle as CO
import glue_oracle as GO
from oracle_hold import out as _out, ratio as _ratio, hold_exact

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
TAG = "CONV"
torch.set_num_threads(min(16, torch.get_num_threads()))


def _api():
    from autoregressive_diffusion_amd import ops, _lib
    return ops, _lib


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rn(gen, *shape, scale=1.0, lim=8.0):
    return (torch.randn(*shape, generator=gen) * scale).clamp(-lim, lim).to(BF16)


def _probe(gen, *shape, density=0.3, top=2):
    """Integer-exact probe: sparse ternary times small integers."""
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    keep = torch.rand(*shape, generator=gen) < density
    return (sign * keep * torch.randint(1, top + 1, shape, generator=gen)).to(BF16)


def _pow2(gen, *shape, signed=False):
    v = 2.0 ** torch.randint(0, 3, shape, generator=gen).float()
    if signed:
        v = v * (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1)
    return v


def _g(t):
    return None if t is None else t.to(DEV).contiguous()


def _weights_gpu(p):
    """A packed weight on the GPU with 128 zero rows behind it (tiles of every kernel stay inside the allocation)."""
    taps, CoutP, CinP = p.shape
    buf = torch.zeros(taps * CoutP * CinP + 128 * CinP, dtype=BF16, device=DEV)
    buf[:p.numel()] = p.reshape(-1).to(DEV)
    return buf


# ---------------------------------------------------------------------------------------------------------------------
# census

_KEY = re.compile(r"^(\w+)(?:<(.*)>)?(?: \[(.*)\])?$")
_CONV_KERNELS = ("conv_fwd_kernel", "conv_glds_kernel", "conv_stream_kernel", "conv_plain_stream_kernel", "conv1x1_glds_kernel",
                 "conv1x1_few_kernel", "conv_eval1_kernel", "conv_wgrad_kernel", "conv_wgrad_glds_kernel", "conv_wgrad_stream_kernel",
                 "wgrad1x1_glds_kernel")


def _launched(before, after):
    """[(kernel, template arguments, tag)] of the conv launches between two census peeks."""
    got = []
    for k, n in after.items():
        if n - before.get(k, 0) > 0:
            m = _KEY.match(k)
            if m and m.group(1) in _CONV_KERNELS:
                got.append((m.group(1), (m.group(2) or "").replace(" ", ""), m.group(3) or ""))
    return sorted(set(got))


def _assert_aim(case, before, after, aim):
    """aim = (kernel, prefix of its template arguments without blanks[, tag]): the launches were of that instantiation and of no
    other conv kernel.  Where the aim names a tag, the census key of every one of them carries it; where it names none, no key
    carries a tag other than the `nt-stores` of the non-temporal policy (a plain launch counted under `pair-rows` fails)."""
    got = _launched(before, after)
    assert got and all(k == aim[0] and a.startswith(aim[1]) for k, a, _ in got), (case, "aimed at", aim, "launched", got)
    tags = (aim[2],) if len(aim) > 2 else ("", "nt-stores")
    assert all(tag in tags for _, _, tag in got), (case, "aimed at", aim, "launched", got)


# ---------------------------------------------------------------------------------------------------------------------
# forward and data gradient
#
# mode: plain  S = 1, no context                                   train      S = 2, ctx = x itself (row stride 2 T), coff (-2, -1), fill 1
#       train_sep  the same with the clean frames in a buffer of their own   dgrad   S = 2, ctx = dy3 [B T], coff (+2, +1), fill 0, wb packing
#       eval1  S = T = 1 against a cached pair, coff (0, 1)        append     S = 1, ctx = [cached pair | x] per sequence, coff (0, 1)
#       e1_store / e1_ctx / e1_read  eval1 with ctx_prod_mode 1 / 3 / 2     pair, pair_store, pair_read  the same with ctx_rows = B / 2
#       cat  taps 1, x = [cat_w1 x | cat_w2 x2] with act_out
# epi: none | silu (pitched escale) | mpsum0 (clip = 0) | mpsum_far (a clip nothing reaches) | mpsum_hit (a clip many elements exceed)
# (name, mode, B, T, H, W, Cin, Cout, taps, epi, aim, nt)
FWD = [
    # conv_fwd_kernel <S, TAPS, CK, NT, HAS_CTX, PW, NW, ACTB>: register-staged
    ("st_8x8", "train", 2, 3, 8, 8, 24, 40, 9, "none", ("conv_fwd_kernel", "2,9,32,2,true,8,"), False),
    ("st_4x4", "train", 2, 3, 4, 4, 24, 24, 9, "silu", ("conv_fwd_kernel", "2,9,32,1,true,4,"), False),
    ("st_2x2", "train", 2, 5, 2, 2, 24, 8, 9, "mpsum_hit", ("conv_fwd_kernel", "2,9,32,1,true,2,"), False),
    ("st_8x4", "train", 2, 3, 8, 4, 24, 40, 9, "mpsum_far", ("conv_fwd_kernel", "2,9,32,2,true,4,"), False),
    ("st_8x8_clip0", "train", 2, 3, 8, 8, 24, 40, 9, "mpsum0", ("conv_fwd_kernel", "2,9,32,2,true,8,"), False),
    ("st_8x8_dgrad", "dgrad", 2, 3, 8, 8, 40, 24, 9, "none", ("conv_fwd_kernel", "2,9,32,1,true,8,"), False),
    ("st_plain_odd", "plain", 1, 3, 16, 16, 24, 40, 9, "mpsum0", ("conv_fwd_kernel", "1,9,32,2,false,16,"), False),
    ("st_1x1_36", "plain", 1, 5, 6, 6, 64, 40, 1, "silu", ("conv_fwd_kernel", "1,1,64,"), False),
    ("st_splitk", "train", 2, 3, 8, 8, 64, 24, 9, "none", ("conv_fwd_kernel", "2,9,32,1,true,8,"), False),    # 4 tiles: K dealt to 6 slices + the reduce launch
    ("st_1x1_nt2", "plain", 1, 40, 16, 16, 64, 128, 1, "silu", ("conv_fwd_kernel", "1,1,64,2,"), False),
    ("st_1x1_nt3", "plain", 1, 60, 16, 16, 64, 96, 1, "silu", ("conv_fwd_kernel", "1,1,64,3,"), False),
    # conv_glds_kernel <NT, PW, NW, MT, WC, CTX, RES>, 16-pixel-wide tiles
    ("g16_32_72", "train", 2, 3, 16, 16, 32, 72, 9, "silu", ("conv_glds_kernel", "1,16,8,1,1,true,true"), True),
    ("g16_64_64", "train", 2, 5, 32, 16, 64, 64, 9, "mpsum_hit", ("conv_glds_kernel", "2,16,8,1,1,true,false"), True),
    ("g16_64_40", "train", 2, 3, 16, 16, 64, 40, 9, "mpsum_far", ("conv_glds_kernel", "2,16,8,1,1,true,false"), True),
    ("g16_32_64", "train", 2, 3, 16, 16, 32, 64, 9, "mpsum0", ("conv_glds_kernel", "2,16,8,1,1,true,false"), True),
    ("g16_dgrad", "dgrad", 2, 3, 16, 16, 64, 32, 9, "none", ("conv_glds_kernel", "1,16,8,1,1,true,false"), True),
    ("g16_plain", "plain", 1, 4, 16, 16, 32, 40, 9, "none", ("conv_glds_kernel", "2,16,8,1,1,false"), True),
    # ... 8x8 images, two frames per tile
    ("g8_32_64", "train", 2, 3, 8, 8, 32, 64, 9, "silu", ("conv_glds_kernel", "1,8,8,1,2,true"), True),
    ("g8_64_64", "train", 2, 5, 8, 8, 64, 64, 9, "mpsum_hit", ("conv_glds_kernel", "1,8,8,1,2,true"), True),
    ("g8_far_40", "train", 2, 3, 8, 8, 32, 40, 9, "mpsum_far", ("conv_glds_kernel", "1,8,8,1,2,true"), True),
    ("g8_clip0", "train", 2, 3, 8, 8, 64, 64, 9, "mpsum0", ("conv_glds_kernel", "1,8,8,1,2,true"), True),
    ("g8_dgrad", "dgrad", 2, 3, 8, 8, 64, 64, 9, "none", ("conv_glds_kernel", "1,8,8,1,2,true"), True),
    ("g8_plain", "plain", 1, 6, 8, 8, 32, 64, 9, "mpsum_far", ("conv_glds_kernel", "1,8,8,1,2,false"), True),
    # conv_stream_kernel <ALIAS>
    ("s_alias", "train", 2, 3, 16, 16, 32, 32, 9, "mpsum_hit", ("conv_stream_kernel", "true"), True),
    ("s_sep_8", "train_sep", 2, 3, 16, 16, 32, 8, 9, "silu", ("conv_stream_kernel", "false"), True),
    ("s_far_24", "train", 2, 3, 16, 16, 32, 24, 9, "mpsum_far", ("conv_stream_kernel", "true"), True),
    ("s_12x16_T1", "train", 2, 1, 12, 16, 32, 32, 9, "none", ("conv_stream_kernel", "true"), True),
    ("s_segments", "train", 2, 19, 16, 16, 32, 32, 9, "mpsum0", ("conv_stream_kernel", "true"), True),      # two segments: 10 + 9 frames
    ("s_dgrad", "dgrad", 2, 3, 16, 16, 32, 32, 9, "none", ("conv_stream_kernel", "false"), True),
    # conv_plain_stream_kernel: 512 tiles of 8 x 16 at the least
    ("ps_64", "plain", 1, 64, 32, 32, 32, 32, 9, "silu", ("conv_plain_stream_kernel", ""), True),
    ("ps_65_24", "plain", 1, 65, 32, 32, 32, 24, 9, "mpsum_far", ("conv_plain_stream_kernel", ""), True),
    # conv1x1_glds_kernel: >= 8192 positions, a ragged last tile, ragged Cout
    ("c1g_136", "plain", 1, 9, 32, 29, 64, 136, 1, "mpsum0", ("conv1x1_glds_kernel", "false"), True),
    # conv1x1_few_kernel
    ("few_1", "plain", 1, 1, 6, 7, 64, 40, 1, "none", ("conv1x1_few_kernel", ""), False),
    ("few_2", "plain", 1, 2, 6, 7, 24, 64, 1, "mpsum_hit", ("conv1x1_few_kernel", ""), False),
    # conv_eval1_kernel <CO>
    ("ev_8x8", "eval1", 2, 1, 8, 8, 64, 64, 9, "silu", ("conv_eval1_kernel", "16"), False),
    ("ev_16x8", "eval1", 1, 1, 16, 8, 64, 40, 9, "mpsum_far", ("conv_eval1_kernel", "16"), False),
    ("ev_co32", "eval1", 5, 1, 16, 16, 32, 256, 9, "none", ("conv_eval1_kernel", "32"), False),              # more than 128 32-channel workgroups
    # S = 1 with a context through conv3x3_pick<1, true>: the prefill / several-frame append (edm2/conv.py: ctx = [cached pair | the
    # T new frames], row stride T + 2) and the one-frame launches the streaming kernel refuses (as the rollout issues them: ctx = the
    # pair alone, ctx_T = 2)
    ("ap_16x16", "append", 2, 3, 16, 16, 24, 40, 9, "silu", ("conv_fwd_kernel", "1,9,32,2,true,16,"), False),
    ("ap_8x8", "append", 2, 5, 8, 8, 64, 64, 9, "mpsum_hit", ("conv_fwd_kernel", "1,9,32,2,true,8,"), False),      # T > 2: frames read frames of the same call
    ("ap_4x4", "append", 3, 2, 4, 4, 32, 24, 9, "mpsum_far", ("conv_fwd_kernel", "1,9,32,1,true,4,"), False),
    ("ap_2x2_T1", "append", 2, 1, 2, 2, 64, 8, 9, "none", ("conv_fwd_kernel", "1,9,32,1,true,2,"), False),         # W = 2 (a split-K pair)
    ("ap_c24_T1", "append", 2, 1, 8, 8, 24, 40, 9, "silu", ("conv_fwd_kernel", "1,9,32,2,true,8,"), False),        # Cin % 32 != 0
    ("ap_ones", "append", 2, 2, 8, 8, 32, 32, 9, "none", ("conv_fwd_kernel", "1,9,32,1,true,8,"), False),          # the first prefill: the cached pair is all ones
    # conv_eval1_kernel, ctx_prod_mode 1 / 3 / 2: NP = (Cin / 32) * (3 / 2 / 1) phases through the four-slot ring
    ("e1_store", "e1_store", 2, 1, 8, 8, 64, 40, 9, "mpsum_far", ("conv_eval1_kernel", "16"), False),
    ("e1_ctx_32", "e1_ctx", 3, 1, 16, 8, 32, 64, 9, "none", ("conv_eval1_kernel", "16"), False),                    # NP = 2; x and out are None
    ("e1_ctx_96", "e1_ctx", 1, 1, 8, 8, 96, 24, 9, "none", ("conv_eval1_kernel", "16"), False),                     # NP = 6: the ring wraps with ph0 = 1
    ("e1_read_32", "e1_read", 2, 1, 8, 16, 32, 64, 9, "silu", ("conv_eval1_kernel", "16"), False),                  # NP = 1
    ("e1_read_160", "e1_read", 1, 1, 8, 8, 160, 24, 9, "mpsum_hit", ("conv_eval1_kernel", "16"), False),            # NP = 5
    ("e1_read_co32", "e1_read", 5, 1, 16, 16, 32, 256, 9, "none", ("conv_eval1_kernel", "32"), False),              # 160 workgroups
    # ... the guided pair (ctx_rows = B / 2): rows >= B / 2 walk the own phases only
    ("pair_silu", "pair", 4, 1, 8, 8, 64, 64, 9, "silu", ("conv_eval1_kernel", "16", "pair-rows"), False),          # NP 6 and 2 in one launch
    ("pair_mpsum", "pair", 2, 1, 16, 8, 32, 40, 9, "mpsum_hit", ("conv_eval1_kernel", "16", "pair-rows"), False),
    ("pair_store", "pair_store", 4, 1, 8, 8, 32, 32, 9, "none", ("conv_eval1_kernel", "16", "pair-rows"), False),
    ("pair_read", "pair_read", 6, 1, 8, 8, 96, 64, 9, "silu", ("conv_eval1_kernel", "16", "pair-rows"), False),
    ("pair_co32", "pair", 6, 1, 16, 16, 32, 256, 9, "none", ("conv_eval1_kernel", "32", "pair-rows"), False),       # 192 workgroups
    # the two-source 1x1 conv (x2 / act_out); Cin = (C1, C2)
    ("cat_few_ragged", "cat", 1, 1, 6, 7, (24, 16), 40, 1, "none", ("conv1x1_few_kernel", ""), False),             # 42 positions, the split inside a k-step
    ("cat_few_512", "cat", 2, 1, 8, 8, (256, 256), 64, 1, "mpsum_hit", ("conv1x1_few_kernel", ""), False),         # two rounds per wave, act_out dealt over 2 blocks
    ("cat_staged", "cat", 1, 5, 16, 16, (40, 24), 224, 1, "none", ("conv_fwd_kernel", "1,1,64,"), False),           # 280 32 x 32 tiles: more than the few-tile kernel takes
]
_PROBE_TA, _PROBE_TB = 2.0, 1.0


_ONE_FRAME = {"eval1": 0, "e1_store": 1, "e1_ctx": 3, "e1_read": 2, "pair": 0, "pair_store": 1, "pair_read": 2}   # mode -> ctx_prod_mode


def _ctx_phases(mode):
    return 1 if mode in ("plain", "cat") else 3


def _cin(Cin):
    """Input channels of a row: the `cat` rows give them as (C1, C2)."""
    return sum(Cin) if isinstance(Cin, tuple) else Cin


def _pair_rows(mode, B):
    """ctx_rows of a row."""
    return B // 2 if mode.startswith("pair") else 0


def fwd_u(row):
    """u of bound_out for a row: (27 Cin | taps Cin) + 12 + 16 roundings -- and 9 Cin + 12 + 16 for the frames that walk the own taps
    only: every frame of a ctx_prod_mode 2 launch and the 2-D rows of a pair (then u is a column over the frames)."""
    name, mode, B, T, H, W, Cin, Cout, taps = row[:9]
    full, own = CO.u_fwd(taps * _cin(Cin) * _ctx_phases(mode), 12), CO.u_fwd(taps * _cin(Cin), 12)
    R = _pair_rows(mode, B)
    if _ONE_FRAME.get(mode) == 2:
        return own
    if R:
        u = torch.full((B, 1, 1, 1), full, dtype=torch.float64)
        u[R:] = own
        return u
    return full


def _pow2w(gen, density, *shape):
    """Probe weights: signed powers of two in {1, 2, 4}, sparse where the case needs it."""
    return (_pow2(gen, *shape, signed=True) * (torch.rand(*shape, generator=gen) < density)).to(BF16)


def probe_densities(mode, taps, Cin, ones=False):
    """Densities (x, own weight, context weight) of a probe case, chosen so that mag stays below 256 (test_conv_oracle.py asserts
    it).  The frames in front of a training sequence are ALL ONES (ctx_fill = 1), and so is the cached pair of the first prefill
    (`ones`): there the context weights alone make up mag, 2 taps Cin of them per output, so they are the sparse side; elsewhere
    the budget is shared between x and the weights.  The first source of a `cat` row is doubled on the way in (cat_w1 = 2)."""
    k1 = taps * Cin
    if mode in ("plain", "cat"):
        dw_own, dw_ctx, load = 0.25, 0.0, k1 * 0.25 * 2.33 * (2 if mode == "cat" else 1)
    else:
        dw_ctx = min(0.25, 64.0 / (2 * k1 * 2.33 * 2)) if mode in ("train", "train_sep") or ones else 0.25
        dw_own = min(0.5, 4 * dw_ctx)
        load = k1 * dw_own * 2.33 * 4 + 2 * k1 * dw_ctx * 2.33 * 2
    return min(0.3, 48.0 / (load * 1.5)), dw_own, dw_ctx


_PROBE_CAT_W = (2.0, 1.0)


def _mp_cat_w(C1, C2, t=0.3):
    """The weights mp_cat gives its two sources (utils.py:128-134), as the float32 values a launch is handed.  (t = 0.3, not the
    decoder's 0.5: two sources of equal width would both get 1.0 there, and a swapped pair would not show.)"""
    n = ((C1 + C2) / ((1 - t) ** 2 + t ** 2)) ** 0.5
    return tuple(float(torch.tensor(v, dtype=torch.float32)) for v in (n * (1 - t) / C1 ** 0.5, n * t / C2 ** 0.5))


def fwd_inputs(row, probe):
    """CPU tensors of one forward case: what the launch reads, and the keyword arguments conv_oracle.conv_fwd takes.  The rows of a
    guided pair (ctx_rows = R = B / 2): x and res hold B independent rows; ctx, coef_*, escale and ctx_prod hold R."""
    name, mode, B, T, H, W, Cin, Cout, taps, epi, aim, nt = row
    C1 = Cin[0] if mode == "cat" else 0
    Cin = _cin(Cin)
    S = 2 if mode in ("train", "train_sep", "dgrad") else 1
    N = B * S * T
    R = _pair_rows(mode, B)
    Nc = R if R else N                                # frames with a coefficient pair and an emb-scale row of their own
    pm = _ONE_FRAME.get(mode, 0)
    gen = _gen(sum(map(ord, name)) + (7 if probe else 0))
    K = taps * Cin * _ctx_phases(mode)
    dx, dw_own, dw_ctx = probe_densities(mode, taps, Cin, ones=name == "ap_ones")
    val = (lambda *s, **k: _probe(gen, *s, density=dx)) if probe else (lambda *s, scale=1.0: _rn(gen, *s, scale=scale))
    wrand = lambda *s: _rn(gen, *s, scale=K ** -0.5)
    wval = (lambda *s: _pow2w(gen, dw_own, *s)) if probe else wrand
    wval_ctx = (lambda *s: _pow2w(gen, dw_ctx, *s)) if probe else wrand
    d = dict(B=B, S=S, T=T, H=H, W=W, Cin=Cin, Cout=Cout, taps=taps)
    d["x"] = val(N, H, W, C1 if C1 else Cin)
    d["x2"], d["x_split"], d["cat_w"] = None, 0, (1.0, 1.0)
    if mode == "cat":
        d["x2"], d["x_split"] = val(N, H, W, Cin - C1), C1
        d["cat_w"] = _PROBE_CAT_W if probe else _mp_cat_w(C1, Cin - C1)
    CoutP, CinP = CO.roundup(Cout, 32), CO.roundup(Cin, 64)
    pad = wval(2 * taps, CoutP, CinP)                 # live values in the padded ROWS
    pack = CO.pack_wb if mode == "dgrad" else CO.pack_wf
    # pack_wb packs a (cout, cin) weight into [taps][cin][cout]: hand it the weight of the forward conv this launch is the adjoint of
    shape = (Cin, Cout, taps) if mode == "dgrad" else (Cout, Cin, taps)
    d["w_own"] = pack(wval(*shape), pad[:taps])
    d["ctx"] = d["w_ctx"] = d["coef_own"] = d["coef_ctx"] = d["ctx_prod"] = None
    d["ctx_bstride"], d["ctx_T"], d["coff"], d["ctx_fill"] = 0, 0, (0, 0), 0.0
    d["ctx_prod_mode"], d["ctx_rows"] = pm, R
    if _ctx_phases(mode) == 3:
        d["w_ctx"] = pack(wval_ctx(shape[0], shape[1], 2, taps), pad)
        n = torch.arange(Nc)
        if probe:
            d["coef_own"], d["coef_ctx"] = 2.0 ** (n % 3).float(), 2.0 ** ((n + 1) % 2).float()
        else:
            d["coef_own"], d["coef_ctx"] = 0.35 + 0.6 * torch.rand(Nc, generator=gen), 0.2 + 0.7 * torch.rand(Nc, generator=gen)
        if mode == "train":
            d["ctx"], d["ctx_bstride"], d["ctx_T"], d["coff"], d["ctx_fill"] = "x", 2 * T, T, (-2, -1), 1.0
        elif mode == "train_sep":
            d["ctx"] = d["x"].reshape(B, 2, T, H, W, Cin)[:, 0].reshape(B * T, H, W, Cin).clone()
            d["ctx_bstride"], d["ctx_T"], d["coff"], d["ctx_fill"] = T, T, (-2, -1), 1.0
        elif mode == "dgrad":
            d["ctx"], d["ctx_bstride"], d["ctx_T"], d["coff"], d["ctx_fill"] = val(B * T, H, W, Cin), T, T, (2, 1), 0.0
            if not probe:
                d["coef_ctx"][T:2 * T] = 0.0          # the context gradient reaches the clean slot only (ops._clean_selector)
        elif mode == "append":
            pair = torch.ones(B, 2, H, W, Cin, dtype=BF16) if name == "ap_ones" else val(B, 2, H, W, Cin)
            d["coff"] = (0, 1)
            if T == 1:                                # one frame: its context IS the cached pair
                d["ctx"], d["ctx_bstride"], d["ctx_T"] = pair.reshape(B * 2, H, W, Cin), 2, 2
            else:
                d["ctx"] = torch.cat([pair, d["x"].reshape(B, T, H, W, Cin)], 1).reshape(B * (T + 2), H, W, Cin)
                d["ctx_bstride"], d["ctx_T"] = T + 2, T + 2
        else:                                         # the one-frame modes: a cached pair per sequence that has one
            d["ctx"], d["ctx_bstride"], d["ctx_T"], d["coff"], d["ctx_fill"] = val((R if R else B) * 2, H, W, Cin), 2, 2, (0, 1), 0.0
        if pm == 2:
            # the kept product is the TEST's: fp32 of unit scale (small integers in the probe), never a launch's output; the launch
            # must read neither the pair nor its weights
            d["ctx"] = d["w_ctx"] = None
            d["ctx_prod"] = _probe(gen, Nc, H, W, Cout).float() if probe else torch.randn(Nc, H, W, Cout, generator=gen)
    d["epi"], d["res"], d["escale"], d["ta"], d["tb"], d["clip"] = CO.EPI_NONE, None, None, 0.0, 0.0, 0.0
    if epi == "silu":
        d["epi"] = CO.EPI_EMB_SILU
        d["escale"] = (2.0 ** torch.randint(-1, 2, (Nc, Cout), generator=gen).float()) if probe else 1 + 0.3 * torch.randn(Nc, Cout, generator=gen)
    elif epi.startswith("mpsum"):
        d["epi"] = CO.EPI_MPSUM
        d["res"] = val(N, H, W, Cout)
        d["ta"], d["tb"] = (_PROBE_TA, _PROBE_TB) if probe else (0.8, 0.6)
    return d


_FWD_KW = ("B", "S", "T", "H", "W", "Cin", "Cout", "taps", "coef_own", "coef_ctx", "ctx_bstride", "ctx_T", "coff", "ctx_fill", "epi", "res",
           "escale", "ta", "tb", "ctx_prod", "ctx_prod_mode", "ctx_rows", "x2", "x_split", "cat_w")


def fwd_reference(d, out_bf16=None, clip=None):
    kw = {k: d[k] for k in _FWD_KW}
    ctx = d["x"] if isinstance(d["ctx"], str) else d["ctx"]
    return CO.conv_fwd(d["x"], ctx, d["w_own"], d["w_ctx"], clip=d["clip"] if clip is None else clip, out_bf16=out_bf16, **kw)


def pick_clip(d, epi, probe):
    """The clip of a case, from the unclipped reference: mpsum_far = 4 x the largest |q| (a power of two: nothing reaches it),
    mpsum_hit = about half the largest |q| (bf16-representable; many elements exceed it by far more than their bound)."""
    if epi not in ("mpsum_far", "mpsum_hit"):
        return 0.0
    top = float(fwd_reference(d, clip=0.0)["out"][0].abs().max())
    if epi == "mpsum_far":
        return float(2.0 ** (2 + max(0, int(top)).bit_length()))
    return float(max(1, int(top / 2))) if probe else float(torch.tensor(top / 2).to(BF16))


def _run_fwd(row, probe):
    ops, _lib = _api()
    name, mode, B, T, H, W, Cin, Cout, taps, epi, aim, nt = row
    case = name + ("/probe" if probe else "")
    d = fwd_inputs(row, probe)
    d["clip"] = pick_clip(d, epi, probe)
    Cin = d["Cin"]
    S, N = d["S"], B * d["S"] * T
    pm, R = d["ctx_prod_mode"], d["ctx_rows"]
    Nc = R if R else N
    CoutP, CinP = CO.roundup(Cout, 32), CO.roundup(Cin, 64)

    def rows_of(t):
        """A tensor of the cached half on the GPU.  In a pair launch: the leading R rows of a buffer 2 R rows long whose tail is NaN
        -- a 2-D row that indexes it by its own b comes back NaN."""
        if t is None or not R:
            return _g(t)
        t = t.reshape(R, -1)
        buf = torch.full((2 * R, t.shape[1]), float("nan"), dtype=t.dtype, device=DEV)
        buf[:R] = t.to(DEV)
        return buf[:R]
    xg = None if pm == 3 else _g(d["x"])              # (mode 3: x and out may be NULL)
    if pm == 2:                                       # the pair and its weights are there and must not be read
        ctxg = torch.full((2 * Nc * 2, H, W, Cin), float("nan"), dtype=BF16, device=DEV)
        wc = _weights_gpu(torch.full((18, CoutP, CinP), float("nan"), dtype=BF16))
    else:
        ctxg = xg if isinstance(d["ctx"], str) else rows_of(d["ctx"])
        wc = None if d["w_ctx"] is None else _weights_gpu(d["w_ctx"])
    wo = _weights_gpu(d["w_own"])
    out = None if pm == 3 else _out(N, H, W, Cout)
    # (the raw output beside EPI_MPSUM is optional; the 1x1 launches go without it: conv1x1_few_kernel declines it)
    out2 = _out(N, H, W, Cout) if d["epi"] == CO.EPI_EMB_SILU or (d["epi"] == CO.EPI_MPSUM and taps == 9) else None
    ctx_out = _out(B * T, H, W, Cout) if mode in ("train", "train_sep") else None
    # the kept product: an fp32 output (modes 1, 3: NaN-prefilled) or the test's own input (mode 2), 2 R rows long in a pair launch
    prod_buf = prod = None
    if pm:
        prod_buf = _out(2 * R if R else N, H, W, Cout, dtype=torch.float32)
        prod = prod_buf[:Nc]
        if pm == 2:
            prod.copy_(d["ctx_prod"].to(DEV))
    x2g = _g(d["x2"])
    act_out = _out(N, H, W, Cin) if x2g is not None else None
    esc = None
    if d["escale"] is not None:                       # a column block of a wider matrix: row pitch Cout + 72, 4 floats in
        wide = torch.full((2 * R if R else N, Cout + 72), float("nan"), device=DEV)
        wide[:Nc, 4:4 + Cout] = d["escale"].to(DEV)
        esc = wide[:Nc, 4:4 + Cout]
    flag = torch.zeros(1, dtype=torch.int32, device=DEV) if d["clip"] > 0 else None
    before = ops.census_peek()
    ops._conv_launch(xg, ctxg, wo, wc, out, rows_of(d["coef_own"]), rows_of(d["coef_ctx"]), B, S, T, H, W, Cin, CinP, Cout,
                     CoutP, taps, ctx_bstride=d["ctx_bstride"], ctx_T=d["ctx_T"], coff=d["coff"], ctx_fill=d["ctx_fill"],
                     epi=d["epi"], res=_g(d["res"]), escale=esc, out2=out2, ta=d["ta"], tb=d["tb"], clip=d["clip"], ctx_out=ctx_out,
                     clip_flag=flag, ctx_prod=prod, ctx_prod_mode=pm, ctx_rows=R, x2=x2g, act_out=act_out, x_split=d["x_split"],
                     cat_w=d["cat_w"])
    torch.cuda.synchronize()
    after = ops.census_peek()
    _assert_aim(case, before, after, aim)
    if name in ("st_splitk", "ap_2x2_T1"):            # the slices' launch + the launch that adds them
        assert sum(n - before.get(k, 0) for k, n in after.items() if k.startswith("conv_fwd_kernel")) == 2, case
    r = fwd_reference(d, out_bf16=out)
    u = fwd_u(row)
    tensors = []
    if out is not None:
        tensors.append(("out", out, CO.bound_out(r["out"], u)))
    if d["epi"] == CO.EPI_EMB_SILU:
        tensors.append(("out2", out2, CO.bound_act(r["out2"])))
    elif out2 is not None:
        tensors.append(("out2", out2, CO.bound_out(r["out2"], u)))
    if ctx_out is not None:
        tensors.append(("ctx_out", ctx_out, CO.bound_out(r["ctx_out"], u)))
    if pm in (1, 3):
        tensors.append(("ctx_prod", prod, CO.bound_ctx_prod(r["ctx_prod"], Cin)))
    if act_out is not None:
        tensors.append(("act_out", act_out, GO.bound_bf16(*r["act_out"])))
    for tname, got, bound in tensors:
        ref = r[tname][0]
        if probe and not (tname == "out2" and d["epi"] == CO.EPI_EMB_SILU) and tname != "act_out":
            hold_exact(case, tname, got, ref, TAG)
        else:
            _ratio(case, tname, got, ref, bound, TAG)
    if pm in (1, 3) and R:                            # the product has R rows and no more
        assert bool(torch.isnan(prod_buf[R:]).all()), (case, "ctx_prod was written beyond its ctx_rows rows")
    if flag is not None:
        reports = aim[0] in ("conv_glds_kernel", "conv_stream_kernel")
        if epi == "mpsum_hit":
            assert r["clip_hit"] and int(flag) == 1, (case, "clip_flag", int(flag))
        elif reports:
            assert not r["clip_hit"] and int(flag) == 0, (case, "clip_flag", int(flag))


_NT = [r for r in FWD if r[-1]]
_PLAIN = [r for r in FWD if not r[-1]]
_id = lambda r: r[0]


@pytest.mark.usefixtures("nt_policy")
@pytest.mark.parametrize("probe", [False, True], ids=["random", "probe"])
@pytest.mark.parametrize("row", _NT, ids=_id)
def test_conv_fwd_nt_families(row, probe):
    """The LDS-DMA and streaming families (their stores follow the non-temporal policy): forward and data gradient."""
    _run_fwd(row, probe)


@pytest.mark.parametrize("probe", [False, True], ids=["random", "probe"])
@pytest.mark.parametrize("row", _PLAIN, ids=_id)
def test_conv_fwd_families(row, probe):
    """The register-staged kernels (3x3 at every patch width, 1x1, the split-K pair), the few-tile 1x1 kernel and the one-frame
    cached evaluation -- and the launch forms of the evaluation path: append, ctx_prod_mode 1 / 2 / 3, the guided pair, the
    two-source 1x1 conv."""
    _run_fwd(row, probe)


# (Cin 16: ops.pair_conv_ok is false, the pair goes out as two launches)
PAIR_FALLBACK = ("pair_fallback", "pair", 4, 1, 8, 8, 16, 16, 9, "silu", None, False)


@pytest.mark.parametrize("probe", [False, True], ids=["random", "probe"])
def test_pair_fallback(probe):
    """ops.gated_conv_eval(..., ctx_rows=2) at a shape the one-frame kernel does not take: the cached half and the 2-D half as two
    launches of the register-staged kernel, held to the same ctx_rows restatement with the bounds of the table rows.  With an
    emb-scale the wrapper returns the activation alone, so it is called twice on the same inputs: without `cscale` it returns
    `out` (held to bound_out, exact in the probe); with `cscale` the same two launches -- they are deterministic -- return out2,
    which the restatement derives from that `out` as it does for every other silu row.
    An ops-level case: the wrapper allocates its outputs and takes tensors of exactly ctx_rows rows, so there are no NaN-prefilled
    outputs and no NaN tails behind coef_*, escale and ctx here; those guards are the table rows'."""
    import types
    ops, _lib = _api()
    row = PAIR_FALLBACK
    name, mode, B, T, H, W, Cin, Cout, taps = row[:9]
    case = name + ("/probe" if probe else "")
    d = fwd_inputs(row, probe)
    d["clip"] = 0.0
    R = d["ctx_rows"]
    CoutP, CinP = CO.roundup(Cout, 32), CO.roundup(Cin, 64)
    pw2, pw3 = (types.SimpleNamespace(wf=_weights_gpu(d[k]), cout=Cout, CinP=CinP, CoutP=CoutP) for k in ("w_own", "w_ctx"))
    xg = _g(d["x"])
    assert not ops.pair_conv_ok(xg, pw2)
    ctxg, coefs = _g(d["ctx"]).reshape(R, 2, H, W, Cin), (_g(d["coef_own"]), _g(d["coef_ctx"]))
    want = ("1,9,32,1,true,8,", "1,9,32,1,false,8,")  # the cached half, the 2-D half
    got = {}
    for tname, kw in (("out", {}), ("out2", dict(cscale=_g(d["escale"])))):
        before = ops.census_peek()
        got[tname] = ops.gated_conv_eval(xg, None, pw2, pw3, B, 1, ctxg, coefs=coefs, ctx_rows=R, **kw)
        torch.cuda.synchronize()
        launched = _launched(before, ops.census_peek())
        assert all(k == "conv_fwd_kernel" and a.startswith(want) and tag == "" for k, a, tag in launched), (case, launched)
        assert all(any(a.startswith(w) for _, a, _ in launched) for w in want), (case, launched)
    r = fwd_reference(d, out_bf16=got["out"])
    if probe:
        hold_exact(case, "out", got["out"], r["out"][0], TAG)
    else:
        _ratio(case, "out", got["out"], r["out"][0], CO.bound_out(r["out"], fwd_u(row)), TAG)
    _ratio(case, "out2", got["out2"], r["out2"][0], CO.bound_act(r["out2"]), TAG)


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient
#
# kind: own    one group: every frame against itself (optionally scaled)
#       gated  three groups: own (scale) + the context taps coff -2 / -1 into the 18-deep slabs (fill 1; scale unless `stream`)
#       ctx1   one context group (coff -1, tap0 9 of 18): taps 0..8 of its slabs stay zero
# (name, kind, B, T, H, W, Cin, Cout, taps, cap (0: ops._nsplit_cap), pad_, scaled, aim)
WGRAD = [
    # conv_wgrad_kernel <TAPS, PW, CT, IT>
    ("wr_16_forced", "gated", 2, 3, 16, 16, 32, 40, 9, 0, -1, True, ("conv_wgrad_kernel", "9,16,1,1")),
    ("wr_8", "gated", 2, 3, 16, 8, 24, 24, 9, 0, 0, True, ("conv_wgrad_kernel", "9,8,1,1")),
    ("wr_4", "gated", 2, 3, 8, 4, 64, 40, 9, 0, 0, True, ("conv_wgrad_kernel", "9,4,2,2")),
    ("wr_2", "own", 1, 33, 4, 2, 24, 8, 9, 0, 0, True, ("conv_wgrad_kernel", "9,2,1,1")),
    ("wr_1x1", "own", 1, 3, 6, 7, 24, 40, 1, 0, 0, True, ("conv_wgrad_kernel", "1,16,1,1")),
    ("wr_1x1_22", "own", 1, 5, 6, 6, 64, 72, 1, 0, -1, False, ("conv_wgrad_kernel", "1,16,2,2")),
    # conv_wgrad_glds_kernel <CT, IT, NG, PW>
    ("wg_16", "gated", 2, 3, 16, 16, 64, 40, 9, 0, 0, True, ("conv_wgrad_glds_kernel", "2,2,1,16")),
    ("wg_8", "gated", 2, 3, 8, 8, 32, 64, 9, 0, 0, True, ("conv_wgrad_glds_kernel", "1,1,1,8")),
    ("wg_own", "own", 1, 5, 8, 32, 24, 24, 9, 0, 0, False, ("conv_wgrad_glds_kernel", "1,1,1,16")),
    ("wg_ctx1", "ctx1", 2, 3, 16, 16, 32, 32, 9, 0, 0, True, ("conv_wgrad_glds_kernel", "1,1,1,16")),
    ("wg_many", "own", 1, 40, 16, 16, 32, 32, 9, 4, 0, True, ("conv_wgrad_glds_kernel", "1,1,1,16")),       # 80 tiles on 4 columns
    # conv_wgrad_stream_kernel <PH>: inside its slab-count condition, and just outside (falls back to the LDS-DMA kernel)
    ("ws_in", "gated", 2, 3, 16, 16, 32, 32, 9, 0, 0, False, ("conv_wgrad_stream_kernel", "4")),
    ("ws_ph8", "gated", 2, 3, 16, 16, 32, 24, 9, 4, 0, False, ("conv_wgrad_stream_kernel", "8")),            # 8 tiles of 4 x 16 > 4 slabs >= 4 tiles of 8 x 16
    ("ws_out", "gated", 2, 3, 16, 16, 32, 32, 9, 2, 0, False, ("conv_wgrad_glds_kernel", "1,1,1,16")),
    # wgrad1x1_glds_kernel <NG>
    ("w1_glds", "own", 1, 3, 6, 7, 64, 72, 1, 0, 0, False, ("wgrad1x1_glds_kernel", "")),
]


def wgrad_groups(row, probe):
    """[(group dict)] of one weight-gradient case: CPU tensors and the geometry of every group; groups 'c0' / 'c1' share the 18-deep
    slabs of the context weight."""
    name, kind, B, T, H, W, Cin, Cout, taps, cap, pad_, scaled, aim = row
    gen = _gen(sum(map(ord, name)) + (7 if probe else 0))
    N = B * 2 * T if kind != "own" else B * T
    P = N * H * W
    # probe densities (mag <= 256, asserted by test_conv_oracle.py): the fill frames of a context group are all ones, so dy is the
    # sparse side there
    if kind == "own":
        ddy = ddx = min(0.3, (40.0 / (P * 5.25)) ** 0.5)
    else:
        ddy = min(0.3, 48.0 / (2 * B * H * W * 3.5))
        ddx = min(0.3, 40.0 / (P * ddy * 5.25))
    val = (lambda *s, dy=False: _probe(gen, *s, density=ddy if dy else ddx)) if probe else (lambda *s, dy=False: _rn(gen, *s))
    sc = (lambda n: 2.0 ** (torch.arange(n) % 3).float()) if probe else (lambda n: 0.3 + 0.6 * torch.rand(n, generator=gen))
    x = val(N, H, W, Cin)
    geo = dict(H=H, W=W, Cin=Cin, Cout=Cout, taps=taps)
    groups = []
    if kind in ("own", "gated"):
        groups.append(dict(geo, key="own", x=x, dy=val(N, H, W, Cout, dy=True), scale=sc(N) if scaled or kind == "gated" else None, B=1, T=N,
                           xb_stride=N, x_T=N, coff=0, fill=0.0, tap0=0, taps_total=taps, slabs="w2"))
    if kind in ("gated", "ctx1"):
        dy3 = val(B * T, H, W, Cout, dy=True)
        for j, coff in enumerate((-2, -1)):
            if kind == "ctx1" and j == 0:
                continue
            groups.append(dict(geo, key=f"c{j}", x=x, dy=dy3, scale=sc(B * T) if scaled else None, B=B, T=T, xb_stride=2 * T, x_T=T,
                               coff=coff, fill=1.0, tap0=9 * j, taps_total=18, slabs="w3"))
    return groups


def wgrad_reference(g):
    return CO.conv_wgrad(g["x"], g["dy"], g["scale"], g["B"], g["T"], g["H"], g["W"], g["Cin"], g["Cout"], g["taps"], g["xb_stride"],
                         g["x_T"], g["coff"], g["fill"], g["tap0"], g["taps_total"])


def _run_wgrad(row, probe):
    ops, _lib = _api()
    name, kind, B, T, H, W, Cin, Cout, taps, cap, pad_, scaled, aim = row
    case = name + ("/probe" if probe else "")
    groups = wgrad_groups(row, probe)
    CoutP, CinP = CO.roundup(Cout, 32), CO.roundup(Cin, 64)
    cap = cap or ops._nsplit_cap(Cin, Cout, taps, gated_pair=kind != "own")
    slabs, nsplits, keep, args = {}, {}, [], []
    xg = _g(groups[0]["x"])
    dyg = {}
    for g in groups:
        if g["slabs"] not in slabs:                   # accumulators: zeroed, as ops._ZeroArena hands them out
            slabs[g["slabs"]] = torch.zeros(cap, CoutP, g["taps_total"], CinP, dtype=BF16, device=DEV)
        if id(g["dy"]) not in dyg:
            dyg[id(g["dy"])] = _g(g["dy"])
        # (one counter per weight, as OnirisWeightDesc.nsplit is: the context groups share theirs)
        g["nsplit"] = nsplits.setdefault(g["slabs"], torch.full((1,), -1, dtype=torch.int32, device=DEV))
        scg = _g(g["scale"])
        keep.append(scg)
        a = _lib.WgradArgs()
        a.x, a.dy, a.dwp, a.scale = ops._p(xg), ops._p(dyg[id(g["dy"])]), ops._p(slabs[g["slabs"]]), ops._p(scg)
        a.nsplit_cap, a.taps_total, a.tap0, a.nsplit_out = cap, g["taps_total"], g["tap0"], ops._p(g["nsplit"])
        a.B, a.T, a.H, a.W, a.Cin, a.CinP, a.Cout, a.CoutP, a.taps = g["B"], g["T"], H, W, Cin, CinP, Cout, CoutP, taps
        a.xb_stride, a.x_T, a.coff, a.fill, a.pad_ = g["xb_stride"], g["x_T"], g["coff"], g["fill"], pad_
        args.append(a)
    before = ops.census_peek()
    ops._wgrad_launch_group(args)
    torch.cuda.synchronize()
    after = ops.census_peek()
    _assert_aim(case, before, after, aim)
    covered = {k: torch.zeros(v.shape[2], dtype=torch.bool) for k, v in slabs.items()}
    for g in groups:
        ns = int(g["nsplit"])
        assert 1 <= ns <= cap, (case, g["key"], "nsplit_out", ns, "cap", cap)
        taps_of = slice(g["tap0"], g["tap0"] + taps)
        covered[g["slabs"]][taps_of] = True
        mine = slabs[g["slabs"]][:, :, taps_of].double().cpu()
        assert bool(torch.isfinite(mine).all()), (case, g["key"], "non-finite slab")
        assert bool((mine[ns:] == 0).all()), (case, g["key"], "a slab at or beyond nsplit_out was written")
        ref, mag = wgrad_reference(g)
        full = lambda t: torch.nn.functional.pad(t[:, taps_of].permute(0, 1, 2), (0, CinP - Cin, 0, 0, 0, CoutP - Cout))
        got = mine[:ns].sum(0)
        positions = g["B"] * g["T"] * H * W
        print(f"{TAG} {case} {g['key']} nsplit_out {ns} of {cap}, chain {CO.wgrad_chain(positions, ns)}")
        if probe:
            hold_exact(case, "dw_" + g["key"], got, full(ref), TAG)
        else:
            bound = CO.bound_wgrad((ref, mag), CO.wgrad_chain(positions, ns), g["scale"] is not None)
            _ratio(case, "dw_" + g["key"], got, full(ref), full(bound), TAG)
    for k, v in slabs.items():
        if bool((~covered[k]).any()):
            assert bool((v[:, :, ~covered[k]].float() == 0).all()), (case, k, "a tap outside every group's [tap0, tap0 + taps) was written")


@pytest.mark.parametrize("probe", [False, True], ids=["random", "probe"])
@pytest.mark.parametrize("row", WGRAD, ids=_id)
def test_conv_wgrad_families(row, probe):
    """Every weight-gradient family through oniris_conv_wgrad_group: the float64 sum of the slabs the launch reports against the
    full sum over positions, the slabs beyond nsplit_out and the taps outside the groups' ranges untouched."""
    _run_wgrad(row, probe)
