"""Bit identity of the attention prologue kernels (csrc/attention_qkv.h) between two builds (profiles/qkv_shared_parts.txt, step 3).

  python scratch/qkv_parts_bits.py run DIR          in a fresh process: every case below on seeded inputs, straight through the lib.oniris_* entry
                                                    points; every output tensor goes to DIR/tensors.pt, the kernel instantiations each case launched
                                                    (ops.census_start / census_stop) to DIR/census.json
  python scratch/qkv_parts_bits.py compare A B ...  torch.equal on every tensor of run A against run B (and of every further pair of runs), no tolerance
                                                    (none of these kernels has atomics), and the census of all runs together against the nine kernels

The library is chosen by ONIRIS_LIB_NAME (autoregressive_diffusion_amd/_lib.py).  ONIRIS_QKV_EVAL_FEW=0 in the environment (read once per
process) sends every oniris_qkv_eval launch to qkv_eval_kernel<KC> instead of qkv_eval_few_kernel: one `run` with it and one without per build.
Outputs start as zeros, so the parts of a ring no kernel writes compare as well.
"""
import json
import os
import sys

import torch

DEV, BF16 = "cuda", torch.bfloat16
EXPECTED = (["qkv_norm_kernel", "qkv_norm_bwd_kernel", "qkv_norm_rope_kernel", "qkv_norm_rope_bwd_kernel", "qkv_norm_rope_eval_kernel",
             "qkv_eval_few_kernel", "rope_kernel", "attn_delta_kernel"] + [f"qkv_eval_kernel<{kc}>" for kc in (64, 128, 256)]
            + ["qkv_eval_few_kernel [pair-rows]"] + [f"qkv_eval_kernel<{kc}> [pair-rows]" for kc in (64, 128, 256)])


def norm_name(n):
    """census key -> 'kernel<args>[ [tag]]' (kernels without template arguments come mangled: _Z<len><name>...)"""
    tag = " [" + n.split(" [", 1)[1] if " [" in n else ""
    n = n.split(" [")[0].replace("void ", "").replace(", ", ",")
    if n.startswith("_Z"):
        digits = "".join(c for c in n[2:4] if c.isdigit())
        n = n[2 + len(digits):2 + len(digits) + int(digits)]
    return n.split("(")[0] + tag


def run(outdir):
    from autoregressive_diffusion_amd import ops
    lib, p, st = ops.lib, ops._p, ops._stream
    os.makedirs(outdir, exist_ok=True)
    out, census = {}, {}
    inv = (1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))).to(DEV)
    scv = ((torch.arange(0, 64, 2) + 0.4 * 64) / (1.4 * 64)).to(DEV)

    def tables(n_pos):
        return [t.contiguous() for t in ops.rope_tables(inv, scv, n_pos, DEV)]

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

    def rnd(g, *shape, scale=1.0):
        return (scale * torch.randn(*shape, generator=g)).to(DEV, BF16)

    def zeros(*shape, dtype=BF16):
        return torch.zeros(*shape, dtype=dtype, device=DEV)

    # ---- the 8-lane kernels: 40 tokens (P = 8, B = 1, T = 5: the last workgroup is partly empty), one head and three
    def lane8(C):
        g = torch.Generator().manual_seed(100 + C)
        ntok, P, T = 40, 8, 5
        cs, sn, sc = tables(T)
        qkv = rnd(g, ntok, 3 * C)
        dq, dk, dv = rnd(g, ntok, C), rnd(g, ntok, C), rnd(g, ntok, C)
        res = {}
        q, k, v = zeros(ntok, C), zeros(ntok, C), zeros(ntok, C)
        ops.check(lib.oniris_qkv_norm(p(qkv), p(q), p(k), p(v), ntok, C, 0, 0, 0, st()), "qkv_norm")
        res.update(norm_q=q, norm_k=k, norm_v=v)
        for tag, tpb, frames, off in (("ring1", 40, 8, 16), ("ring5", 8, 4, 16)):       # one sequence of five frames; five sequences of one frame
            nb, bstride = ntok // tpb, frames * P * C
            q, k, v = zeros(ntok, C), zeros(nb, bstride), zeros(nb, bstride)
            ops.check(lib.oniris_qkv_norm(p(qkv), p(q), p(k), p(v), ntok, C, tpb, bstride, off * 1, st()), "qkv_norm")
            res.update({f"{tag}_q": q, f"{tag}_k": k, f"{tag}_v": v})
        dqkv = zeros(ntok, 3 * C)
        ops.check(lib.oniris_qkv_norm_bwd(p(qkv), p(dq), p(dk), p(dv), p(dqkv), ntok, C, st()), "qkv_norm_bwd")
        res["norm_dqkv"] = dqkv
        q, k, v = zeros(ntok, C), zeros(ntok, C), zeros(ntok, C)
        ops.check(lib.oniris_qkv_norm_rope(p(qkv), p(q), p(k), p(v), p(cs), p(sn), p(sc), ntok, C, P, T, st()), "qkv_norm_rope")
        res.update(rope_q=q, rope_k=k, rope_v=v)
        dqkv = zeros(ntok, 3 * C)
        ops.check(lib.oniris_qkv_norm_rope_bwd(p(qkv), p(dq), p(dk), p(dv), p(dqkv), p(cs), p(sn), p(sc), ntok, C, P, T, st()), "qkv_norm_rope_bwd")
        res["rope_dqkv"] = dqkv
        return res

    # ---- qkv_norm_rope_eval_kernel: B = 2, P = 8, a ring of 4 frames with 2 committed, position 2
    def rope_eval(C):
        g = torch.Generator().manual_seed(200 + C)
        B, P, cap, n = 2, 8, 4, 2
        cs, sn, sc = tables(n + 1)
        qkv = rnd(g, B * P, 3 * C)
        q, k, v, kr = zeros(B * P, C), zeros(B, cap * P * C), zeros(B, cap * P * C), zeros(B, cap * P * C)
        ops.check(lib.oniris_qkv_norm_rope_eval(p(qkv), p(q), p(k), p(v), p(kr), p(cs), p(sn), p(sc), B * P, C, P, cap * P * C, n * P, n, st()),
                  "qkv_norm_rope_eval")
        return dict(q=q, k=k, v=v, kr=kr)

    # ---- rope_kernel: L = 40 (a partial 64-token tile, partial 8-token groups of the transposed copy), two heads
    def rope(B, strided):
        g = torch.Generator().manual_seed(300 + B)
        frames, P, C = 5, 8, 128
        L = frames * P
        xs = L * C + (192 if strided else 0)
        x = rnd(g, B, xs)
        tabs = tables(frames)
        res = {}
        for mode in range(5):
            for want_r, want_t in ((1, 0), (0, 1), (1, 1)):
                xr = zeros(B, xs + (64 if strided else 0)) if want_r else None
                xt = zeros(B * (C // 64) * 64, L) if want_t else None
                ops.check(lib.oniris_rope(p(x), p(xr), p(xt), *(p(t) for t in tabs), mode, B, frames, P, C, 0, frames, xs if strided else 0,
                                          xs + 64 if strided else 0, st()), "rope")
                if want_r:
                    res[f"m{mode}r{want_r}t{want_t}_xr"] = xr
                if want_t:
                    res[f"m{mode}r{want_r}t{want_t}_xt"] = xt
        return res

    # ---- attn_delta_kernel: three heads, with and without the negated row constants (and once with the transposed dO)
    def delta():
        g = torch.Generator().manual_seed(400)
        B, heads, L = 1, 3, 40
        C = heads * 64
        dout, o = rnd(g, B * L, C), rnd(g, B * L, C)
        lse = torch.randn(B, heads, L, generator=g).to(DEV)
        res = {}
        d0 = zeros(B, heads, L, dtype=torch.float32)
        ops.check(lib.oniris_attn_bwd_prep(p(dout), p(o), p(d0), None, None, None, B, heads, L, C, st()), "attn_bwd_prep")
        d1, neg, dt = zeros(B, heads, L, dtype=torch.float32), zeros(2, B, heads, L, dtype=torch.float32), zeros(B * heads * 64, L)
        ops.check(lib.oniris_attn_bwd_prep(p(dout), p(o), p(d1), p(dt), p(lse), p(neg), B, heads, L, C, st()), "attn_bwd_prep")
        return dict(delta=d0, delta_neg=d1, neg=neg, doutt=dt)

    # ---- oniris_qkv_eval / _pair: conv + norm (+ rotation) in one launch.  40 tokens: ragged against the 32-token tiles of the few-tile
    # kernel; 136: one full 128-token tile plus 8 rows (three waves of the last tile hold no valid row)
    def qkv_eval(ntok, C, form):
        g = torch.Generator().manual_seed(500 + ntok + C)
        x = rnd(g, ntok, C)
        w = rnd(g, 3 * C, C, scale=C ** -0.5)
        cap, n = 4, 2
        if form == "frame":              # no tables, dense outputs
            q, k, v = zeros(ntok, C), zeros(ntok, C), zeros(ntok, C)
            ops.check(lib.oniris_qkv_eval(p(x), p(w), p(q), p(k), p(v), None, None, None, None, ntok, C, C, 0, 0, 0, 0, st()), "qkv_eval")
            return dict(q=q, k=k, v=v)
        cs, sn, sc = tables(n + 1)
        if form == "ring":               # sequences of one 8-token frame behind two committed frames
            P = 8
            nb, bstride = ntok // P, cap * P * C
            q, k, v, kr = zeros(ntok, C), zeros(nb, bstride), zeros(nb, bstride), zeros(nb, bstride)
            ops.check(lib.oniris_qkv_eval(p(x), p(w), p(q), p(k), p(v), p(kr), p(cs), p(sn), p(sc), ntok, C, C, P, bstride, n * P, n, st()), "qkv_eval")
            return dict(q=q, k=k, v=v, kr=kr)
        P, split = 4, ntok // 2          # pair: the first half as "ring" with 4-token frames, the second half as "frame"
        nb, bstride = split // P, cap * P * C
        q, k, v, kr = zeros(split, C), zeros(nb, bstride), zeros(nb, bstride), zeros(nb, bstride)
        q2, k2, v2 = zeros(ntok - split, C), zeros(ntok - split, C), zeros(ntok - split, C)
        ops.check(lib.oniris_qkv_eval_pair(p(x), p(w), p(q), p(k), p(v), p(kr), p(cs), p(sn), p(sc), ntok, split, C, C, P, bstride, n * P, n,
                                           p(q2), p(k2), p(v2), st()), "qkv_eval_pair")
        return dict(q=q, k=k, v=v, kr=kr, q2=q2, k2=k2, v2=v2)

    for C in (64, 192):
        case(f"lane8(C{C})", lambda: lane8(C))
        case(f"rope_eval(C{C})", lambda: rope_eval(C))
    for B, strided in ((1, False), (2, True)):
        case(f"rope(B{B},strided{int(strided)})", lambda: rope(B, strided))
    case("delta", delta)
    for ntok, Cs in ((40, (64, 256, 320)), (136, (64, 128, 256, 320))):
        for C in Cs:
            for form in ("ring", "frame", "pair"):
                case(f"qkv_eval(n{ntok},C{C},{form})", lambda: qkv_eval(ntok, C, form))

    torch.save(out, os.path.join(outdir, "tensors.pt"))
    json.dump(census, open(os.path.join(outdir, "census.json"), "w"), indent=1)
    reached = sorted({k for v in census.values() for k in v})
    print(f"{len(out)} tensors of {len(census)} cases; ONIRIS_QKV_EVAL_FEW={os.environ.get('ONIRIS_QKV_EVAL_FEW', '(unset)')}; launched: {reached}")


def compare(dirs):
    """dirs = A B [A2 B2 ...]: run A against run B, A2 against B2 (the pair with ONIRIS_QKV_EVAL_FEW=0), ..."""
    ok, reached = len(dirs) >= 2 and len(dirs) % 2 == 0, set()
    for a, b in zip(dirs[0::2], dirs[1::2]):
        ta, tb = torch.load(os.path.join(a, "tensors.pt")), torch.load(os.path.join(b, "tensors.pt"))
        ca, cb = json.load(open(os.path.join(a, "census.json"))), json.load(open(os.path.join(b, "census.json")))
        reached |= {k for c in (ca, cb) for v in c.values() for k in v}
        nonfinite = sum(int((~torch.isfinite(x)).sum()) for t in (ta, tb) for x in t.values())
        zeros = [k for k, x in ta.items() if not x.any()]
        differ = []
        for k in sorted(set(ta) & set(tb)):
            if not torch.equal(ta[k], tb[k]):
                differ.append(k)
                ne = ta[k] != tb[k]
                print(f"  {k}: {int(ne.sum())} of {ne.numel()} elements differ, largest |difference| {float((ta[k] - tb[k]).abs().max()):.3e} "
                      f"(largest |element| {float(ta[k].abs().max()):.3e})")
        print(f"{a} | {b}: tensors {len(ta)} / {len(tb)}, the same names: {sorted(ta) == sorted(tb)}; the same census per case: {ca == cb}; "
              f"elements compared: {sum(x.numel() for x in ta.values())}; non-finite: {nonfinite}; all-zero tensors: {zeros}")
        print(f"  tensors that differ: {differ}")
        ok = ok and sorted(ta) == sorted(tb) and ca == cb and not differ and not nonfinite and not zeros
    print(f"kernels launched by these runs: {sorted(reached)}")
    missing = [k for k in EXPECTED if k not in reached]
    print(f"of the nine kernels, the three KC and their pair-rows launches, not reached: {missing}")
    ok = ok and not missing
    print("bit-identical, every kernel reached:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    sys.exit(run(sys.argv[2]) if sys.argv[1] == "run" else compare(sys.argv[2:]))
