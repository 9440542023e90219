"""The expectations of tests/fp32_oracle.py see what they claim to see.  No kernel runs here.  Each fault below is planted in the
float32 restatement of the operation (model_f32 for attention, torch's float32 convolution on the CPU for the convs) and compared
with the float64 expectation under the bound tests/test_fp32_stages_gpu.py asserts: the planted result must exceed the bound at
least FAULT_MARGIN = 3 times over somewhere, the unplanted one must stay within it everywhere.

Also here, being torch code that runs on the CPU: fp32.resample and fp32.rope against float64 restatements."""
import math

import pytest
import torch
import torch.nn.functional as F

import fp32_oracle as FO
from oracle import oniris_oracle as O

_cases = {}


def count_case(cid):
    """(mask name, kernel arguments, allowed, inputs, float64 reference) of a count-probe case, computed once."""
    if not _cases:
        for c, name, kw, build in FO.count_cases():
            _cases[c] = [name, kw, build, None, None]
    c = _cases[cid]
    if c[3] is None:
        c[2] = c[2]()
        c[3] = FO.count_probe(FO.COUNT_BH, FO.COUNT_D, c[2])
        c[4] = FO.reference(*c[3], c[2])
    return c


COUNT_IDS = [c for c, _, _, _ in FO.count_cases()]


def closed_form_train(T, P, le=False):
    """The closed form attn_allowed (csrc/fp32.hip) evaluates for mask_mode 2; le: the fault 'kt <= fpb (qt / fpb)'."""
    tok = torch.arange(2 * T * P)
    qf, kf = tok[:, None] // P, tok[None, :] // P
    qs, ks, qt, kt = qf // T, kf // T, qf % T, kf % T
    fpb = 1 if P >= 128 else 128 // P
    edge = fpb * (qt // fpb)
    past = (kt <= edge) if le else (kt < edge)
    return ((qs == 0) & (ks == 0) & (kt <= qt)) | ((qs == 1) & (ks == 0) & past) | ((qs == 1) & (ks == 1) & (kt == qt))


def count_errors(got, ref):
    """(out: worst |err|, dv: worst |err|, dq / dk: worst |err| / largest |dv|) against the float64 reference."""
    top = float(ref["dv"].abs().max())
    e = {n: float((got[n].double() - ref[n]).abs().max()) for n in FO.NAMES}
    return e["out"], e["dv"], max(e["dq"], e["dk"]) / top


# ----------------------------------------------------------------------------------------------------------------------
# masks and count probes

@pytest.mark.parametrize("P,T", FO.TRAIN_COUNT_CASES)
def test_training_mask_from_the_definitions(P, T):
    """Table AND mask_mod from the package's own definitions equals the oracle's dense mask and the kernel's closed form, at every
    count-probe shape; the lengths are the ones the cases are chosen for."""
    allowed = FO.train_allowed(T, P)
    assert allowed.shape == ((1024, 1024) if P == 256 else (512, 512))
    assert torch.equal(allowed, torch.from_numpy(O.train_allowed_tokens(T, P)))
    assert torch.equal(allowed, closed_form_train(T, P))
    assert bool(allowed.any(1).all())
    # the block table only takes pairs away below 128-token frames
    assert torch.equal(allowed, FO.train_mask_mod_only(T, P)) == (P >= 128)


@pytest.mark.parametrize("tq,n,P", FO.CAUSAL_CASES)
def test_causal_mask_from_the_definition(tq, n, P):
    allowed = FO.causal_allowed(tq, n, P)
    qi, kj = torch.arange(tq * P)[:, None], torch.arange((n + tq) * P)[None, :]
    assert allowed.shape == (tq * P, (n + tq) * P)
    assert torch.equal(allowed, kj // P <= qi // P + n)
    assert {(2, 3, 20): (40, 100), (2, 1, 9): (18, 27), (3, 0, 50): (150, 150)}[(tq, n, P)] == tuple(allowed.shape)


@pytest.mark.parametrize("cid", COUNT_IDS)
def test_count_probe_reference_and_model(cid):
    """The float64 reference of a count probe IS the counts; the float32 model alone stays within 2^-20 (out) and 2^-8 (dv
    absolute; dq, dk relative to the largest |dv|), a quarter of what the GPU test allows the kernel."""
    name, kw, allowed, inp, ref = count_case(cid)
    out, dv = FO.count_expectation(FO.COUNT_D, allowed)
    assert float((ref["out"] - out).abs().max()) < 1e-12 and float((ref["dv"] - dv).abs().max()) < 1e-9
    assert float(ref["dq"].abs().max()) < 1e-9 * float(dv.max())
    # every row attends at least one key and the scores are one constant
    assert int(allowed.sum(1).min()) >= 1
    s = (inp[0].double() @ inp[1].double().transpose(-1, -2))
    assert float((s - s[:, :1, :1]).abs().max()) == 0.0
    e_out, e_dv, e_zero = count_errors(FO.model_f32(*inp, allowed), ref)
    print(f"FP32 oracle {cid}: model_f32 out {e_out:.2e} (bound {FO.COUNT_OUT_TOL:.2e}), dv {e_dv:.2e}, dq/dk {e_zero:.2e} (bound {FO.MODEL_DV_TOL:.2e})")
    assert e_out <= FO.COUNT_OUT_TOL and e_dv <= FO.MODEL_DV_TOL and e_zero <= FO.MODEL_DV_TOL


def planted_count(cid, mutated, what):
    """model_f32 under `mutated` on the inputs of the true mask.  dv must leave its bound FAULT_MARGIN times over, always.  `out`
    must too wherever the counts say it can: row i of `out` holds the SHARES of the classes j % 64 among the keys of row i, and a
    mutation that keeps every row's shares -- whole frames of a multiple of 64 tokens come or go, or a row whose keys all fall
    into one class gains another of that class -- leaves `out` as it is (asserted: within its bound).  That is why dv, the
    transposed mask weighted so that every pair counts 1, is checked at every element too."""
    name, kw, allowed, inp, ref = count_case(cid)
    assert mutated.shape == allowed.shape and not torch.equal(mutated, allowed), what
    shift = float((FO.count_expectation(FO.COUNT_D, mutated)[0] - FO.count_expectation(FO.COUNT_D, allowed)[0]).abs().max())
    out_sees = shift > 0
    assert not out_sees or shift >= 1.0 / allowed.shape[1] / 2
    e_out, e_dv, _ = count_errors(FO.model_f32(*inp, mutated), ref)
    print(f"FP32 fault [{what}] {cid}: out moves {e_out / FO.COUNT_OUT_TOL:.3g} x bound{'' if out_sees else ' (shares unchanged)'}, "
          f"dv {e_dv / FO.COUNT_DV_TOL:.3g} x bound")
    assert (e_out >= FO.FAULT_MARGIN * FO.COUNT_OUT_TOL) if out_sees else (e_out <= FO.COUNT_OUT_TOL), (what, cid, e_out)
    assert e_dv >= FO.FAULT_MARGIN * FO.COUNT_DV_TOL, (what, cid, e_dv)
    return out_sees


def flipped_pairs(allowed):
    """For the first, a middle and the last query row: its last allowed key removed (if it has another) and the first key it may
    not see added (if there is one)."""
    Lq = allowed.shape[0]
    pairs = []
    for i in sorted({0, Lq // 2, Lq - 1}):
        on, off = allowed[i].nonzero()[:, 0], (~allowed[i]).nonzero()[:, 0]
        if len(on) > 1:
            pairs.append((i, int(on[-1])))
        if len(off):
            pairs.append((i, int(off[0])))
    return pairs


@pytest.mark.parametrize("cid", COUNT_IDS)
def test_fault_one_pair_flipped(cid):
    allowed = count_case(cid)[2]
    pairs = flipped_pairs(allowed)
    assert pairs
    for i, j in pairs:
        mutated = allowed.clone()
        mutated[i, j] = not bool(allowed[i, j])
        planted_count(cid, mutated, f"pair ({i}, {j}) {'removed' if allowed[i, j] else 'added'}")


@pytest.mark.parametrize("tq,n,P", FO.CAUSAL_CASES)
@pytest.mark.parametrize("step", [-1, 1])
def test_fault_q_frame_off_by_one(tq, n, P, step):
    if n + step < 0:
        step = 1                  # (no frame before the first: the prefill case is moved forwards both times)
    qi, kj = torch.arange(tq * P)[:, None], torch.arange((n + tq) * P)[None, :]
    planted_count(f"causal-{tq}on{n}-P{P}", kj // P <= qi // P + n + step, f"q_frame_off {n} -> {n + step}")


@pytest.mark.parametrize("P,T", FO.TRAIN_COUNT_CASES)
def test_fault_noisy_rows_see_one_clean_frame_too_many(P, T):
    assert planted_count(f"train-P{P}-T{T}", closed_form_train(T, P, le=True), "kt <= fpb (qt / fpb)") == (P % 64 != 0)


@pytest.mark.parametrize("P,T", [c for c in FO.TRAIN_COUNT_CASES if c[0] < 128])
def test_fault_mask_mod_without_the_table(P, T):
    """Below 128-token frames only: from there on the table takes nothing away (test_training_mask_from_the_definitions)."""
    planted_count(f"train-P{P}-T{T}", FO.train_mask_mod_only(T, P), "mask_mod without the block table")


def test_faults_under_the_random_input_bound():
    """The same four faults with random inputs: some row of `out` and of dv leaves RANDOM_BOUND_FACTOR x the model's own noise
    FAULT_MARGIN times over, the unplanted model is (by construction) a quarter of the bound."""
    tq, n, P = FO.CAUSAL_CASES[0]
    causal = FO.causal_allowed(tq, n, P)
    qi, kj = torch.arange(tq * P)[:, None], torch.arange((n + tq) * P)[None, :]
    flip = causal.clone()
    flip[tq * P - 1, 0] = False
    Pt, Tt = 16, 16
    train = FO.train_allowed(Tt, Pt)
    plan = [("pair (last query, key 0) removed", causal, flip), ("q_frame_off - 1", causal, kj // P <= qi // P + n - 1),
            ("kt <= fpb (qt / fpb)", train, closed_form_train(Tt, Pt, le=True)), ("mask_mod without the block table", train, FO.train_mask_mod_only(Tt, Pt))]
    for what, allowed, mutated in plan:
        inp = FO.random_inputs(1, *allowed.shape, 8, seed=11)
        ref = FO.reference(*inp, allowed)
        bounds = FO.random_bounds(ref, FO.model_f32(*inp, allowed))
        got = FO.model_f32(*inp, mutated)
        sig = {t: float(FO.row_error(got[t], ref[t]).max()) / bounds[t] for t in FO.NAMES}
        print(f"FP32 fault [{what}] random inputs: worst row / bound", {t: f"{v:.3g}" for t, v in sig.items()})
        assert all(b > 0 for b in bounds.values())
        assert sig["out"] >= FO.FAULT_MARGIN and sig["dv"] >= FO.FAULT_MARGIN, (what, sig)


# ----------------------------------------------------------------------------------------------------------------------
# convolution

def conv_inputs(N, H, W, Cin, Cout, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    dy = torch.randn(N, Cout, H, W, generator=g)
    return x, w, dy


def worst_ratio(got, want, bound):
    return float(((got.double() - want).abs() / bound.clamp_min(1e-300)).max())


def test_wgrad_terms_is_the_weight_gradient():
    for k in (1, 3):
        x, w, dy = conv_inputs(2, 5, 4, 3, 4, k, 5)
        wd = w.double().requires_grad_(True)
        F.conv2d(x.double(), wd, padding=k // 2).backward(dy.double())
        dw, mag, cnt = FO.wgrad_terms(x.double(), dy.double(), k)
        assert dw.shape == w.shape and float((dw - wd.grad).abs().max()) < 1e-12
        assert bool((mag >= dw.abs()).all())
        # the centre tap sees every position, a corner tap loses one row and one column
        assert int(cnt[0, 0, k // 2, k // 2]) == 2 * 5 * 4 and (k == 1 or int(cnt[0, 0, 0, 0]) == 2 * 4 * 3)


def test_conv_faults_tall_image_and_dropped_border_tap():
    """(3, 5, 7), 5 -> 7 channels, 3x3: the float32 convolution stays within (K + 4) u sum|terms| at every element; the batch
    convolved as ONE image of 15 rows (no padding between the images) and a single in-bounds tap left out at one border pixel
    both leave it by far more than three times."""
    N, H, W, Cin, Cout = 3, 5, 7, 5, 7
    x, w, dy = conv_inputs(N, H, W, Cin, Cout, 3, 7)
    want, mag = FO.conv_terms(x.double(), w.double())
    bound = FO.element_bound(mag, 9 * Cin)
    clean = F.conv2d(x, w, padding=1)
    assert worst_ratio(clean, want, bound) <= 1.0
    tall = F.conv2d(x.permute(1, 0, 2, 3).reshape(1, Cin, N * H, W), w, padding=1).reshape(Cout, N, H, W).permute(1, 0, 2, 3)
    drop = clean.clone()
    drop[1, :, 0, W - 1] -= w[:, :, 2, 0] @ x[1, :, 1, W - 2]          # tap (+1, -1) of the top right pixel of image 1
    for what, got in (("batch as one tall image", tall), ("one border tap dropped", drop)):
        r = worst_ratio(got, want, bound)
        print(f"FP32 fault [{what}]: {r:.3g} x bound")
        assert r >= FO.FAULT_MARGIN
    # and the data gradient's bound holds for the float32 adjoint
    dwant, dmag = FO.dgrad_terms(dy.double(), w.double())
    assert worst_ratio(F.conv_transpose2d(dy, w, padding=1), dwant, FO.element_bound(dmag, 9 * Cout)) <= 1.0


def test_wgrad_probe_faults():
    """(3, 37, 41), 5 -> 7, 3x3: 4551 positions = one chunk of 4096 + 455 = 28 groups of 16 + 7; position 4096 is column 37 of row
    25 of the third image (a chunk boundary inside an image row).  With the position probes an element has a few dozen terms; the
    kernel dropping the ragged last 7 positions, counting position 4096 twice, or dropping chunk 1 altogether each move some
    element far past (K + nz + 4) u sum|terms|, which the float32 weight gradient holds everywhere."""
    N, H, W, Cin, Cout = 3, 37, 41, 5, 7
    npos = N * H * W
    assert npos == 4551 and FO.wgrad_chunks(npos) == 2 and npos - 4096 == 28 * 16 + 7
    assert divmod(4096 - 2 * H * W, W) == (25, 37)
    pos = FO.probe_positions(N, H, W)
    assert {0, npos - 1, 4094, 4095, 4096, 4097} <= set(pos) and set(range(4096 + 448, npos)) <= set(pos) and set(range(4080, 4096)) <= set(pos)
    x = FO.position_probe(N, H, W, Cin, 3)
    assert int((x.abs().sum(1) != 0).sum()) == len(pos)
    _, _, dy = conv_inputs(N, H, W, Cin, Cout, 3, 9)
    want, mag, cnt = FO.wgrad_terms(x.double(), dy.double(), 3)
    assert int(cnt.max()) <= len(pos) and int(cnt[:, :, 1, 1].min()) == len(pos)
    bound = FO.element_bound(mag, cnt, extra=FO.wgrad_chunks(npos))
    f32 = lambda weights: FO.wgrad_terms(x, dy * FO.position_weights(N, H, W, weights), 3)[0]
    assert worst_ratio(f32({}), want, bound) <= 1.0
    faults = {"last ragged group dropped": {p: 0.0 for p in range(4096 + 448, npos)},
              "position 4096 counted twice": {4096: 2.0},
              "position 4095 counted twice": {4095: 2.0},
              "chunk 1 dropped": {p: 0.0 for p in range(4096, npos)}}
    for what, weights in faults.items():
        r = worst_ratio(f32(weights), want, bound)
        print(f"FP32 fault [{what}]: {r:.3g} x bound, {len(pos)} probe positions")
        assert r >= FO.FAULT_MARGIN
    # dense input (every element a sum over all 4551 positions: what a single position cannot be seen in): the bound holds too
    xd, _, _ = conv_inputs(N, H, W, Cin, Cout, 3, 13)
    want, mag, cnt = FO.wgrad_terms(xd.double(), dy.double(), 3)
    assert int(cnt[:, :, 1, 1].min()) == npos
    assert worst_ratio(FO.wgrad_terms(xd, dy, 3)[0], want, FO.element_bound(mag, cnt, extra=2)) <= 1.0


# ----------------------------------------------------------------------------------------------------------------------
# fp32.resample, fp32.rope (torch code of the fp32 path)

def resample_f64(x, f, mode):
    """edm2/utils.py resample: depthwise conv2d (stride 2) with f f^T / sum(f)^2, or conv_transpose2d with 4 times that filter."""
    f = torch.tensor([float(v) for v in f], dtype=torch.float64)
    pad = (len(f) - 1) // 2
    f = f / f.sum()
    c = x.shape[1]
    k = torch.outer(f, f)[None, None].repeat(c, 1, 1, 1)
    if mode == "down":
        return F.conv2d(x.double(), k, groups=c, stride=2, padding=pad)
    return F.conv_transpose2d(x.double(), 4 * k, groups=c, stride=2, padding=pad)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 6, 4), (1, 1, 1, 1)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("f", [[1, 1], [1, 3, 3, 1]], ids=["f11", "f1331"])
@pytest.mark.parametrize("mode", ["down", "up"])
def test_resample_against_the_filter_formula(shape, f, mode):
    from autoregressive_diffusion_amd import fp32
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape)))
    try:
        want = resample_f64(x, f, mode)
    except RuntimeError:
        # an image smaller than the filter: the formula has no output, fp32.resample must not invent one
        with pytest.raises((RuntimeError, ValueError)):
            fp32.resample(x, f, mode)
        return
    got = fp32.resample(x, f, mode)
    assert got.dtype == torch.float32 and got.shape == want.shape
    r = float((got.double() - want).norm() / want.norm())
    print(f"FP32 resample {mode} {f} {shape} -> {tuple(got.shape)}: rel L2 {r:.2e}")
    assert r <= 1e-6


@pytest.mark.parametrize("training", [False, True], ids=["2-on-5", "training"])
def test_rope_against_the_oracle(training):
    """fp32.rope against oracle.rope_apply in float64 (the fp16 tables are part of the definition and stay fp16).  Bound: 4 x the
    error of rope_apply itself evaluated in float32, per tensor, largest |error| over the elements."""
    from autoregressive_diffusion_amd import fp32
    g = torch.Generator().manual_seed(21)
    c = 16
    inv_freq = 1.0 / (10000 ** (torch.arange(0, c, 2).float() / c))
    scale = (torch.arange(0, c, 2) + 0.4 * c) / (1.4 * c)
    nq, nk = (6, 6) if training else (2, 5)
    q, k = torch.randn(2, 3, nq, 7, c, generator=g), torch.randn(2, 3, nk, 7, c, generator=g)
    want = O.rope_apply(q.double(), k.double(), inv_freq, scale, training)
    own = O.rope_apply(q, k, inv_freq, scale, training)
    got = fp32.rope(q, k, inv_freq, scale, training)
    for name, g_, o_, w_ in zip("qk", got, own, want):
        w_ = w_.flatten(-3, -2)
        assert w_.dtype == torch.float64 and g_.shape == w_.shape and g_.dtype == torch.float32
        e, e_own = float((g_.double() - w_).abs().max()), float((o_.flatten(-3, -2).double() - w_).abs().max())
        print(f"FP32 rope {'training' if training else '2 on 5'} {name}: |err| {e:.2e}, the oracle's own in float32 {e_own:.2e}")
        assert e_own > 0 and e <= 4 * e_own
