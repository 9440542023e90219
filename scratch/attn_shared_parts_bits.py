"""Bit identity of the attention kernels between two builds (profiles/attn_shared_parts.txt, step 3).

  python scratch/attn_shared_parts_bits.py run DIR          in a tree, in a fresh process: every case below on seeded inputs; every output
                                                            (out, lse, dq, dk, dv, dqkv) goes to DIR/tensors.pt, the kernel instantiations each case
                                                            launched (ops.census_start / census_stop) to DIR/census.json
  python scratch/attn_shared_parts_bits.py compare A B [C]  torch.equal on every tensor of runs A and B, no tolerance.  With C: A and B are
                                                            two runs of the PARENT, C the new tree; a tensor that differs between A and B
                                                            is named as not bit-reproducible and compared within 2^-6 of its largest
                                                            element instead (the count-probe tolerance of tests/test_attention_probes_gpu.py)

The library is chosen by ONIRIS_LIB_NAME (autoregressive_diffusion_amd/_lib.py), so one Python tree serves both builds.  Shapes and
knob settings are those of the variant tables of tests/test_attention_probes_gpu.py and of test_frame_attention_core_train.
"""
import json
import os
import sys

import torch

DEV, BF16 = "cuda", torch.bfloat16
EXPECTED = ([f"attn_fwd_kernel<{m},{k}>" for m, k in ((0, 1), (0, 4), (1, 1), (1, 2), (2, 1), (2, 2))]
            + [f"attn_bwd_dq_kernel<{m},{k}>" for m, k in ((0, 1), (1, 1), (1, 2), (2, 1), (2, 2))]
            + [f"attn_bwd_dkv_kernel<{m}>" for m in (0, 1, 2)]
            + [f"attn_fwd_ws_kernel<{m}>" for m in (1, 2)] + [f"attn_bwd_dq_ws_kernel<{m}>" for m in (1, 2)]
            + [f"attn_bwd_dkv_ws_kernel<{m},{k}>" for m in (1, 2) for k in (64, 128)]
            + ["attn_split_reduce_kernel", "attn_dkv_reduce_kernel", "frame_attn_fwd_kernel<1>", "frame_attn_fwd_kernel<2>", "frame_attn_dq_kernel",
               "frame_attn_bwd_kernel", "frame_attn_qkv_fwd_kernel", "frame_attn_qkv_bwd_kernel"])

# (ATTN_PERSISTENT, DKV_ITEM_KEYS, ATTN_DKV_CHUNKS, ATTN_DQ_PERSISTENT, ATTN_DKV_PERSISTENT); None: leave the default
DEFAULTS = (1, None, None, 1, 1)
GRID = (0, 0, 1, 1, 1)
CROSS = ([(1, keys, 1, dq, 1) for keys in (0, 128) for dq in (1, 0)] + [(1, 0, chunks, 1, 0) for chunks in (1, 3)]
         + [(0, 0, chunks, 1, 1) for chunks in (1, 3)])


def norm_name(n):
    return n.split(" [")[0].replace("void ", "").replace(", ", ",").replace("(anonymous namespace)::", "")


class Knobs:
    """set attributes of ops for one case, put them back afterwards"""

    def __init__(self, ops, **kw):
        self.ops, self.kw = ops, {k: v for k, v in kw.items() if v is not None}

    def __enter__(self):
        self.old = {k: getattr(self.ops, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(self.ops, k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            setattr(self.ops, k, v)


def video_knobs(ops, knobs):
    persistent, keys, chunks, dq, dkv = knobs
    return Knobs(ops, ATTN_PERSISTENT=persistent, ATTN_DQ_PERSISTENT=dq, ATTN_DKV_PERSISTENT=dkv, DKV_ITEM_KEYS=keys, ATTN_DKV_CHUNKS=chunks,
                 ATTN_DKV_MIN_L=None if chunks is None else 128)


def frame_knobs(ops, variant, video=DEFAULTS):
    ws = variant == "ws"
    v = 3 if ws else variant
    k = video_knobs(ops, video)
    k.kw.update(FRAME_WS=int(ws), FRAME_KERNEL=min(v, 1), FRAME_BWD_FUSED=int(v in (1, 3)), FRAME_QKV_FUSED=int(v == 3))
    return k


def rope():
    inv = 1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))
    sc = (torch.arange(0, 64, 2) + 0.4 * 64) / (1.4 * 64)
    return inv.to(DEV), sc.to(DEV)


def run(outdir):
    from autoregressive_diffusion_amd import ops
    os.makedirs(outdir, exist_ok=True)
    out, census = {}, {}

    def case(name, fn):
        ops.census_start()
        try:
            res = fn()
            torch.cuda.synchronize()
        finally:
            c = ops.census_stop()
        census[name] = sorted({norm_name(k) for k in c})
        for k, v in res.items():
            out[f"{name}/{k}"] = v.detach().float().cpu().clone()

    def train(kind, N, T, B, P, m, seed):
        g = torch.Generator().manual_seed(seed)
        C = 64 * m
        x = torch.randn(N, P, 3 * C, generator=g).to(DEV, BF16).requires_grad_(True)
        go = torch.randn(N, P, C, generator=g).to(DEV, BF16)
        grads = {}
        core_bwd = ops._attn_core_bwd

        def noting_bwd(*a):                        # dq, dk, dv as the attention kernels leave them, in front of the normalisation's adjoint
            r = core_bwd(*a)
            grads.update(dq=r[0], dk=r[1], dv=r[2])
            return r

        ops._attn_core_bwd = noting_bwd
        try:
            o = ops.attention_train(x, kind, B, T, m, rope() if kind == "video" else None)
            lse = [t for t in o.grad_fn.saved_tensors if t.dtype == torch.float32]       # the forward's row constants, kept for the backward
            o.backward(go)
        finally:
            ops._attn_core_bwd = core_bwd
        assert len(lse) == 1
        return {"out": o, "lse": lse[0], "dqkv": x.grad, **grads}      # (the raw-qkv frame kernels write dqkv only)

    # VideoAttention, training table (mask_mode 2): (B, T, H, m); T = 4 with P = 64 and P = 256 (table blocks of 256 tokens)
    for shape, knobs in ([(s, k) for s in [(1, 8, 4, 2), (1, 16, 8, 2)] for k in CROSS]
                         + [(s, k) for s in [(1, 4, 8, 2), (1, 4, 16, 2), (3, 4, 8, 4), (1, 32, 4, 2)] for k in (DEFAULTS, GRID)]):
        B, T, H, m = shape
        with video_knobs(ops, knobs):
            case(f"video{shape}{knobs}", lambda: train("video", B * 2 * T, T, B, H * H, m, 5 + T + H))
    # FrameAttention, training: frames of 64 / 128 / 256 tokens, odd frame counts (partial last super-block); 16-token frames on the grid kernels
    for (N, P, m), v in ([(c, v) for c in [(5, 64, 2), (13, 64, 4), (5, 128, 1), (3, 256, 2)] for v in (3, 1, 2, 0)]
                         + [((5, 128, 1), "ws"), ((16, 256, 2), "ws"), ((3, 16, 1), 0)]):
        with frame_knobs(ops, v):
            case(f"frame({N},{P},{m})v{v}", lambda: train("frame", N, 1, N, P, m, N * P + m))
    # ... on the work lists (block-diagonal table, mask_mode 1) with the other kernel forms: 128-key items, grid kernels (one and two key streams)
    for (N, P, m), video in [((16, 256, 2), (1, 128, 1, 1, 1)), ((16, 256, 2), GRID), ((11, 256, 2), GRID), ((16, 256, 2), (1, 0, 1, 1, 0)),
                             ((11, 256, 2), (1, 0, 1, 1, 0))]:
        with frame_knobs(ops, "ws", video):
            case(f"frame({N},{P},{m})ws{video}", lambda: train("frame", N, 1, N, P, m, N * P + m))

    # evaluation: prefill (table path, dense fall-back with a length that is no multiple of 64, one frame), a second chunk with Lq < Lk,
    # decode with four / one key streams, split-KV decode
    def evaluate(B, P, m, t0, t1, streams, split_min, persistent):
        g = torch.Generator().manual_seed(7 + t0 + P)
        C = 64 * m
        res = {}
        with Knobs(ops, DECODE_STREAMS=streams, DECODE_SPLIT_MIN_KEYS=split_min, ATTN_PERSISTENT=persistent), torch.no_grad():
            x0 = torch.randn(B * t0, P, 3 * C, generator=g).to(DEV, BF16)
            res["prefill"], cache = ops.attention_eval(x0, B, m, rope(), None, True, P)
            if t1:        # t1 new frames against the t0 + t1 cached ones: the causal mask with Lq < Lk (no entry of ops asks for it: a direct launch)
                Lq, Lk = t1 * P, (t0 + t1) * P
                q = (0.3 * torch.randn(B, Lq, C, generator=g)).to(DEV, BF16)
                k, v = (torch.randn(B, Lk, C, generator=g).to(DEV, BF16) for _ in range(2))
                res["chunk"] = torch.empty_like(q)
                res["chunk_lse"] = torch.empty(B, m, Lq, device=DEV)
                a = ops._attn_args(q, k, v, None, None, None, res["chunk"], res["chunk_lse"], None, B, m, Lq, Lk, C, 1, P, 0)
                ops.check(ops.lib.oniris_attn_fwd(ops.ctypes.byref(a), ops._stream()), "attn_fwd")
            x2 = torch.randn(B, P, 3 * C, generator=g).to(DEV, BF16)
            res["decode"], cache = ops.attention_eval(x2, B, m, rope(), cache, True, P)
        return res

    for B, P, m, t0, t1, streams, split_min, persistent in [(2, 64, 1, 4, 0, 1, None, None), (2, 64, 1, 5, 0, 0, None, None), (2, 16, 1, 5, 0, 1, None, None),
                                                            (2, 64, 1, 1, 0, 1, None, None), (2, 64, 1, 4, 2, 1, None, None), (2, 64, 2, 8, 0, 1, 256, None),
                                                            (1, 64, 2, 36, 0, 1, None, None), (1, 64, 2, 32, 2, 0, None, 0), (2, 16, 2, 5, 0, 0, 64, None)]:
        case(f"eval(B{B},P{P},m{m},t{t0}+{t1},streams{streams},split{split_min},persistent{persistent})",
             lambda: evaluate(B, P, m, t0, t1, streams, split_min, persistent))

    torch.save(out, os.path.join(outdir, "tensors.pt"))
    json.dump(census, open(os.path.join(outdir, "census.json"), "w"), indent=1)
    reached = sorted({k for v in census.values() for k in v})
    print(f"{len(out)} tensors of {len(census)} cases; attention instantiations reached: {len([k for k in reached if k in EXPECTED])} of {len(EXPECTED)}")
    print("not reached:", [k for k in EXPECTED if k not in reached])


def compare(a, b, c=None):
    ta, tb = torch.load(os.path.join(a, "tensors.pt")), torch.load(os.path.join(b, "tensors.pt"))
    tc = torch.load(os.path.join(c, "tensors.pt")) if c else None
    ca = json.load(open(os.path.join(a, "census.json")))
    cn = json.load(open(os.path.join(c or b, "census.json")))
    ok = sorted(ta) == sorted(tb) and (tc is None or sorted(tc) == sorted(ta)) and ca == cn
    print(f"tensors: {len(ta)} / {len(tb)}" + (f" / {len(tc)}" if tc else "") + f", the same names: {ok}; the same census per case: {ca == cn}")
    unstable, differ, nonfinite, zeros, elems = [], [], 0, [], 0
    for k in sorted(ta):
        x, new = ta[k], (tc if tc else tb)[k]
        elems += x.numel()
        nonfinite += int((~torch.isfinite(x)).sum()) + int((~torch.isfinite(new)).sum())
        if not x.any():
            zeros.append(k)
        if tc is not None and not torch.equal(x, tb[k]):
            unstable.append(k)
            tol = 2.0 ** -6 * float(x.abs().max())
            if float((x - new).abs().max()) > tol:
                differ.append(k)
        elif not torch.equal(x, new):
            differ.append(k)
            ne = x != new
            print(f"  {k}: {int(ne.sum())} of {x.numel()} elements differ, largest |difference| {float((x - new).abs().max()):.3e} "
                  f"(largest |element| {float(x.abs().max()):.3e}); last-axis positions {sorted(set(ne.nonzero()[:, -1].tolist()))[:16]}")
    reached = sorted({k for v in cn.values() for k in v})
    print(f"elements compared: {elems}; non-finite: {nonfinite}; all-zero tensors: {zeros}")
    if tc is not None:
        print(f"not bit-reproducible in the parent itself (held to 2^-6 of the largest element instead): {unstable}")
    print(f"tensors that differ: {differ}")
    print(f"attention instantiations reached: {[k for k in reached if k in EXPECTED]}")
    print(f"not reached by any case: {[k for k in EXPECTED if k not in reached]}")
    print(f"other kernels launched: {[k for k in reached if k not in EXPECTED]}")
    ok = ok and not differ and not nonfinite and not zeros
    print("bit-identical to the parent:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    sys.exit(run(sys.argv[2]) if sys.argv[1] == "run" else compare(*sys.argv[2:5]))
