"""The count probes of tests/attention_probes.py see what they claim to see.  No kernel runs here: the float64 reference under the
true training mask is compared with the same reference under a MUTATED mask, and the row metric between the two must exceed the
bound the GPU tests assert (COUNT_TOL = 2^-6) at least three times -- for every drawn and every forced position."""
import numpy as np
import pytest
import torch

import attention_probes as AP
from oracle import oniris_oracle as O

SHAPES = [(4, 64), (8, 16), (32, 16), (16, 64), (2, 256)]       # (T, P) of the video cases of test_attention_probes_gpu.py
MARGIN = 3.0
N_DRAWS = 32
# kind (b): ONE query row x 4 aligned keys moves a dv row by 1 / (queries of that class attending the key) = 1/64 at 64- and
# 256-token frames, i.e. 1.0 x COUNT_TOL: not three times.  The smallest aligned group of query rows caught at every position is
# B_ROWS[P] (x 4 keys): one row at 16-token frames, four rows otherwise.
B_ROWS = {16: 1, 64: 4, 256: 4}

_probes = {}


def probe(T, P, cls):
    if (T, P, cls) not in _probes:
        _probes[(T, P, cls)] = AP.HeadProbe(T, P, cls)
    return _probes[(T, P, cls)]


def dv_classes(T):
    return ["frame", "mod64"] if 2 * T <= 32 else ["mod64"]


def forced_rows(T, P):
    """First and last row of a frame (an inner clean one, an inner noisy one), and the clean / noisy seam (qf = T-1, T)."""
    fr = sorted({1, T - 1, T, T + 1, 2 * T - 1})
    return sorted({f * P for f in fr} | {f * P + P - 1 for f in fr})


def forced_pairs(T, P, allowed):
    """For every forced row: its last allowed key and its first allowed key (removed), the key right after an allowed run and the
    key right before one (added), and one allowed + one disallowed key inside the row's LAST LISTED table block."""
    blk = O.train_table(T, P)[2]
    L = allowed.shape[0]
    pairs = []
    for i in forced_rows(T, P):
        row = allowed[i]
        on = np.flatnonzero(row)
        pairs += [(i, int(on[-1])), (i, int(on[0]))]
        edges = np.flatnonzero(row[:-1] != row[1:])
        for e in edges:
            pairs.append((i, int(e if not row[e] else e + 1)))
        b0 = (int(on[-1]) // blk) * blk
        inside = np.arange(b0, min(b0 + blk, L))
        pairs.append((i, int(inside[row[inside]][len(inside[row[inside]]) // 2])))
        off = inside[~row[inside]]
        if len(off):
            pairs += [(i, int(off[0])), (i, int(off[-1]))]
    return sorted(set(pairs))


def single_frame_frames(T, P):
    """Frames whose rows attend their own frame and nothing else.  The training table lists whole blocks of max(P, 128) tokens
    (r = block / P frames): noisy frame f attends the clean frames below floor(f / r) * r and itself, so the noisy frames f < r --
    the first noisy table block -- see themselves only, like the first clean frame."""
    r = O.train_table(T, P)[2] // P
    return [0] + [T + f for f in range(r)]


def inexpressible(kind, i, j, T, P, allowed):
    """Derived from the table alone (mutation() is checked against it at every position): the positions at which a kind would
    leave rows without any key.  (a), (b): none (a row has at least 16 keys).  (c): taking away the only frame a row attends.
    (d): frames under 128 tokens: the 128-row query block that IS the first noisy table block -- the rows that see its last
    64-key tile see nothing else; from 128-token frames on the last tile is a part of the row's own frame."""
    if kind == "c":
        return bool(allowed[i, j]) and (i // P) in single_frame_frames(T, P)
    if kind == "d":
        return P < 128 and T * P <= i < T * P + 128
    return False


def drawn_pairs(kind, T, P, allowed, rng):
    """N_DRAWS allowed pairs (to be removed) and N_DRAWS disallowed pairs (to be added), uniform over the pairs at which `kind` is
    expressible, + how many candidates were passed over because it is not."""
    out, passed_over = [], 0
    for value in (True, False):
        ii, jj = np.nonzero(allowed == value)
        got = 0
        for p in rng.permutation(len(ii)):
            if got == N_DRAWS:
                break
            i, j = int(ii[p]), int(jj[p])
            if inexpressible(kind, i, j, T, P, allowed):
                passed_over += 1
                continue
            out.append((i, j))
            got += 1
        assert got == N_DRAWS
    return out, passed_over


def mutation(kind, i, j, T, P, allowed):
    """(rows, their new mask) of mutation `kind` at pair (i, j), or None if it leaves a row without any key."""
    L = allowed.shape[0]
    if kind == "a":
        rows, keys = np.array([i]), np.array([j])
    elif kind == "b":
        r = B_ROWS[P]
        rows, keys = (i // r) * r + np.arange(r), (j // 4) * 4 + np.arange(4)
    elif kind == "c":
        rows, keys = (i // 16) * 16 + np.arange(16), (j // P) * P + np.arange(P)
    else:                                                   # "d": the query block of row i loses the last 64-key tile it sees
        blk_rows = (i // 128) * 128 + np.arange(128)
        last = max(int(np.flatnonzero(allowed[r])[-1]) for r in blk_rows)
        keys = (last // 64) * 64 + np.arange(64)
        rows = blk_rows[allowed[blk_rows][:, keys].any(1)]
    new = allowed[rows].copy()
    value = False if kind == "d" else not allowed[rows[0], keys[0]]
    new[:, keys] = value
    if not new.any(1).all():
        return None
    assert (new != allowed[rows]).any()
    return rows, new


@pytest.mark.parametrize("T,P", SHAPES)
def test_probes_catch_mask_mutations(T, P):
    allowed = O.train_allowed_tokens(T, P)
    rng = np.random.default_rng(1000 * T + P)
    forced = forced_pairs(T, P, allowed)
    fwd = probe(T, P, "mod64")
    need = MARGIN * AP.COUNT_TOL
    # the inexpressible positions are exactly the derived ones: (1 + r) single-frame frames of P rows with P keys each for (c)
    single = single_frame_frames(T, P)
    one_frame_rows = [i for i in range(2 * T * P) if len(set(np.flatnonzero(allowed[i]) // P)) == 1]
    assert sorted(set(i // P for i in one_frame_rows)) == single and len(one_frame_rows) == len(single) * P
    assert allowed[one_frame_rows].sum() == len(single) * P * P
    skipped, forced_skipped, passed_over, weakest = {}, {}, {}, {}
    for kind in "abcd":
        drawn, passed_over[kind] = drawn_pairs(kind, T, P, allowed, rng)
        skipped[kind] = forced_skipped[kind] = 0
        for n, (i, j) in enumerate(forced + drawn):
            mut = mutation(kind, i, j, T, P, allowed)
            assert (mut is None) == inexpressible(kind, i, j, T, P, allowed), (kind, i, j)
            if mut is None:
                if n < len(forced):
                    forced_skipped[kind] += 1
                else:
                    skipped[kind] += 1
                continue
            rows, new = mut
            if kind == "a":
                o_new, _, _ = fwd.mutated(rows, new)
                sig = AP.HeadProbe.shift(o_new, fwd.out[rows])
                what = "out of the mod-64 probe"
            else:
                sig = 0.0
                for cls in dv_classes(T):
                    pr = probe(T, P, cls)
                    _, keys, dv_new = pr.mutated(rows, new)
                    sig = max(sig, AP.HeadProbe.shift(dv_new, pr.dv[keys]))
                what = "dv fingerprint"
            weakest[kind] = min(weakest.get(kind, np.inf), sig)
            assert sig >= need, (f"T={T} P={P}: mutation ({kind}) at query {i} (frame {i // P}, position {i % P}), key {j} (frame {j // P}) "
                                 f"moves the {what} by only {sig:.3e} < {MARGIN} x {AP.COUNT_TOL:.3e}")
        # positions are drawn where the kind is expressible, so at most 5 % of the drawn ones may be skipped -- for every kind
        assert len(drawn) == 2 * N_DRAWS and skipped[kind] <= 0.05 * len(drawn), (kind, skipped[kind])
        # the forced positions that cannot be expressed are the derived ones and no others: removals on the single-frame frames
        # (the seam's noisy side is one) for (c), the rows of the first noisy table block for (d); none for (a), (b)
        assert forced_skipped[kind] == sum(inexpressible(kind, i, j, T, P, allowed) for (i, j) in forced)
    assert forced_skipped["a"] == forced_skipped["b"] == 0
    # every forced ROW is still tested under (a), (b), (c) at some position (the seam's noisy side by additions under (c)); under (d)
    # the forced rows of the first noisy table block (frames under 128 tokens) are the ones left out
    for kind in "abc":
        assert {i for (i, j) in forced if not inexpressible(kind, i, j, T, P, allowed)} == set(forced_rows(T, P))
    print(f"T={T} P={P} L={2 * T * P}: {len(forced)} forced + {2 * N_DRAWS} drawn positions per kind, weakest signal / COUNT_TOL: "
          + ", ".join(f"({k}) {v / AP.COUNT_TOL:.1f}x" for k, v in weakest.items())
          + f"; drawn positions skipped: {skipped}; candidates passed over as inexpressible: {passed_over}"
          + f"; forced positions inexpressible: {forced_skipped} of {len(forced)}; single-frame frames: {single}")


@pytest.mark.parametrize("T,P,cls", [(4, 64, "frame"), (4, 64, "mod64"), (8, 16, "frame"), (2, 256, "mod64")])
def test_row_update_equals_full_reference(T, P, cls):
    """HeadProbe re-evaluates only the mutated rows; the full autograd reference under the same masks must agree."""
    pr = probe(T, P, cls)
    allowed = pr.allowed
    out, dqkv = AP.reference(pr.x, pr.dO, 1, 1, allowed, AP.identity_rope())
    assert (out.reshape(-1, 64) - pr.out).abs().max() < 1e-12
    g = AP.split_dqkv(dqkv)
    assert (g["dv"].reshape(-1, 64) - pr.dv).abs().max() < 1e-9
    # dq and dk of a count probe vanish (rows of dS sum to zero, K constant; dk parallel to k)
    assert g["dq"].abs().max() < 1e-9 * pr.dv.abs().max() and g["dk"].abs().max() < 1e-9 * pr.dv.abs().max()
    i, j = (T - 1) * P + P - 1, T * P - 1
    for kind in "abcd":
        rows, new = mutation(kind, i, j, T, P, allowed)
        mutated = allowed.copy()
        mutated[rows] = new
        out_m, dqkv_m = AP.reference(pr.x, pr.dO, 1, 1, mutated, AP.identity_rope())
        o_new, keys, dv_new = pr.mutated(rows, new)
        assert (out_m.reshape(-1, 64)[rows] - o_new).abs().max() < 1e-12
        dv_m = AP.split_dqkv(dqkv_m)["dv"].reshape(-1, 64)
        assert (dv_m[keys] - dv_new).abs().max() < 1e-9
        rest = np.setdiff1d(np.arange(2 * T * P), keys.numpy())
        assert (dv_m[rest] - pr.dv[rest]).abs().max() < 1e-9


def test_identity_rope_leaves_q_and_k_unchanged():
    """The count probes rest on it: O.rope_apply under inv_freq = 0, scale = 1 is the identity in float64, in training layout
    (clean T, noisy T) and in evaluation layout (fewer query frames than key frames)."""
    g = torch.Generator().manual_seed(3)
    inv, sc = AP.identity_rope()
    q, k = torch.randn(2, 3, 8, 16, 64, generator=g, dtype=torch.float64), torch.randn(2, 3, 8, 16, 64, generator=g, dtype=torch.float64)
    qr, kr = O.rope_apply(q, k, inv, sc, True)
    assert qr.dtype == torch.float64 and torch.equal(qr, q) and torch.equal(kr, k)
    qr, kr = O.rope_apply(q[:, :, -1:], k, inv, sc, False)
    assert torch.equal(qr, q[:, :, -1:]) and torch.equal(kr, k)
    # and the probe's scores are the constant 8 the issue's range argument assumes
    x, _ = AP.count_probe(1, 8, 16, ["frame", "mod64"])
    qq, kk, _ = AP.prepared_qkv(x.double(), 1, 2, (inv, sc), True)
    s = qq @ kk.transpose(-1, -2) / 8.0
    assert (s - 8.0).abs().max() < 2e-2 and (s - s[..., :1, :1]).abs().max() < 1e-12


def test_bf16_model_noise_of_count_probes_is_under_the_bound():
    """The modelled rounding (bf16 P, operands, results; float32 sums) keeps every count-probe row within COUNT_TOL / 2."""
    for (T, P) in SHAPES:
        allowed = O.train_allowed_tokens(T, P)
        classes = AP.head_classes(2, 2 * T)
        x, dO = AP.count_probe(1, 2 * T, P, classes, allowed)
        out, dqkv = AP.reference(x, dO, 1, 2, allowed, AP.identity_rope())
        mo, mg = AP.model_bf16(x, dO, 1, 2, allowed, AP.identity_rope())
        w = [AP.worst_rows(mo, out, 2, 2 * T), AP.worst_rows(AP.split_dqkv(mg)["dv"], AP.split_dqkv(dqkv)["dv"], 2, 2 * T)]
        print(f"T={T} P={P}: modelled noise out / dv per head", [[round(v, 5) for v, _ in ww] for ww in w])
        assert max(v for ww in w for v, _ in ww) <= AP.COUNT_TOL / 2
