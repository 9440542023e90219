"""The rectangular kv table of t > 1 frames appended to a non-empty cache (ops.append_mask_table) against the brute-force mask
allowed[q, k] = (k // P) <= n + (q // P): every listed block holds an allowed pair, every block that holds one is listed, ascending,
at most 64 per row, and None exactly in the fall-back cases.  CPU only."""
import numpy as np
import pytest

NS = (1, 2, 3, 4, 5, 30, 31)
TS = (2, 3, 4, 5)
PS = (16, 64, 128, 256)
MAX_COLS = 64                 # the grid kernels hold a table row in one VGPR: one entry per lane (block_list, csrc/attention_parts.h)


def brute_force(n, t, P):
    q = np.arange(t * P)[:, None]
    k = np.arange((n + t) * P)[None, :]
    return (k // P) <= n + (q // P)


def block_of(P):
    return P if P >= 128 else 128            # oniris_infer_mask's choice


def expected_blocks(n, t, P):
    """Per query table block of the call: the key blocks with at least one allowed pair, from the brute-force mask."""
    allowed = brute_force(n, t, P)
    blk = block_of(P)
    Lq, Lk = allowed.shape
    rows = []
    for r in range(-(-Lq // blk)):
        sub = allowed[r * blk:(r + 1) * blk]
        rows.append([c for c in range(-(-Lk // blk)) if sub[:, c * blk:(c + 1) * blk].any()])
    return rows


def falls_back(n, t, P):
    """The one-shot prefill's fall-backs (t*P < 128; t*P % 128 != 0 at P < 128) and the 64-blocks-per-row limit."""
    if t * P < 128 or (P < 128 and (t * P) % 128 != 0):
        return True
    return max(len(r) for r in expected_blocks(n, t, P)) > MAX_COLS


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("t", TS)
@pytest.mark.parametrize("n", NS)
def test_append_table_matches_brute_force(n, t, P):
    from autoregressive_diffusion_amd import ops
    tab = ops.append_mask_table(n, t, P)
    if falls_back(n, t, P):
        assert tab is None
        return
    assert tab is not None
    num, idx, blk = tab
    want = expected_blocks(n, t, P)
    assert blk == block_of(P)
    assert num.dtype == np.int32 and idx.dtype == np.int32
    assert num.shape == (len(want),) and idx.shape[0] == len(want)
    assert idx.shape[1] == max(len(r) for r in want) <= MAX_COLS
    for r, blocks in enumerate(want):
        listed = [int(c) for c in idx[r, :num[r]]]
        assert listed == blocks, (r, listed, blocks)          # every block with an allowed pair, nothing else, ascending


def test_the_cap_is_a_condition():
    """(30, 2, 64): Lk = 2048 is 16 blocks per row -- a table; past 64 listed blocks of 128 tokens there is none."""
    from autoregressive_diffusion_amd import ops
    num, idx, blk = ops.append_mask_table(30, 2, 64)
    assert blk == 128 and idx.shape == (1, 16) and list(num) == [16]
    assert ops.append_mask_table(62, 2, 128) is not None and ops.append_mask_table(62, 2, 128)[1].shape[1] == 64
    assert ops.append_mask_table(63, 2, 128) is None
    assert ops.append_mask_table(200, 2, 64) is None


def test_straddling_query_block_lists_a_superset():
    """n*P no multiple of the block (n = 1, P = 64): the only query block holds frames 1 and 2 and lists key blocks 0 and 1; the
    second one ends past the 192 keys."""
    from autoregressive_diffusion_amd import ops
    num, idx, blk = ops.append_mask_table(1, 2, 64)
    assert blk == 128 and list(num) == [2] and idx.tolist() == [[0, 1]]


def test_bad_sizes():
    from autoregressive_diffusion_amd import ops
    for bad in ((-1, 2, 64), (1, 0, 64), (1, 2, 0)):
        with pytest.raises(ValueError):
            ops.append_mask_table(*bad)
