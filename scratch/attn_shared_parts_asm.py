"""Compiler output of attention.hip in two trees, kernel by kernel (profiles/attn_shared_parts.txt, step 2).

  hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Iinclude -Wno-unused-result -mllvm -amdgpu-mfma-vgpr-form=1 \
        --cuda-device-only -S -fuse-cuid=none -Rpass-analysis=kernel-resource-usage \
        autoregressive_diffusion_amd/csrc/attention.hip -o X.s 2> X.remarks                                   (in each tree)
  python scratch/attn_shared_parts_asm.py PARENT.s PARENT.remarks NEW.s NEW.remarks

Per kernel: whole body byte-identical or not; resources of both builds; counts of the instructions the change must not move; the multiset of floating-point opcodes (a product that is
fused into a sum in one build and not in the other is a different result bit); and for the span from the first to the last v_mfma ("main loop": in the persistent kernels that is a whole work item, fill and epilogue
included) whether it is identical, identical up to register numbers, the same opcode sequence, or none of these (then the opcode
multiset is compared too); and the same classes for every innermost loop that holds MFMAs (a backward branch to a label with no
other backward branch inside: the tile / block loops), matched in order.  Exit status 1 when a condition of step 2 fails.
"""
import collections
import re
import subprocess
import sys

COUNTED = ("v_mfma", "ds_read_b64_tr_b16", "buffer_load_lds", "v_exp_f32", "v_cvt_pk_bf16_f32")


def kernels(path):
    """mangled name -> list of body lines"""
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s+; @", line)
        if m:
            name, body = m.group(1), []
        elif name and line.startswith(".Lfunc_end"):
            out[name], name = body, None
        elif name:
            body.append(line)
    return out


def resources(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
            out[name] = {}
        else:
            out[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def instrs(body):
    """instruction lines without comments; an LDS-DMA (buffer_load ... lds, here inside inline asm) gets the opcode buffer_load_lds"""
    out = []
    for l in body:
        t = l.split(";")[0].strip()
        if re.match(r"^\.LBB\d+_\d+:", t):
            out.append(t)
            continue
        if not t or t.startswith(".") or t.endswith(":") or t.startswith("//"):
            continue
        if t.startswith("buffer_load") and t.endswith(" lds"):
            t = "buffer_load_lds " + t.split(None, 1)[1]
        out.append(t)
    return out


def stats(ins):
    ops = [i.split()[0] for i in ins if not i.endswith(":")]
    return dict(lines=len(ops), **{c: sum(1 for o in ops if o.startswith(c)) for c in COUNTED})


FLOAT_OPS = re.compile(r"^v_(pk_)?(fma|fmac|fmamk|fmaak|mac|mad|mul|add|sub|exp|log|rcp|rsq|sqrt|cvt|max|min|dot)\w*_(f32|f16|bf16)")


PK_FLOAT = re.compile(r"^v_pk_(fma|mul|add)_f32")
ALL_READS = re.compile(r"^(global_store|global_atomic|flat_store|buffer_store|scratch_store|ds_write|v_cmp|v_readlane|v_readfirstlane|s_|exp)")
READS_DEST = re.compile(r"^(v_fmac|v_mac|v_pk_fmac|v_dot\w*c_|v_movrel)|d16|sdwa")


def vregs(operand):
    """VGPR numbers an operand names"""
    out = []
    for a, b, c in re.findall(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]", operand):
        out += [int(a)] if a else list(range(int(b), int(c) + 1))
    return out


def operands(t):
    rest = t.split(None, 1)[1] if " " in t else ""
    return [o.strip() for o in re.split(r"\s+[a-z_0-9]+:", rest)[0].split(",")]


def modifier(t, name, n):
    m = re.search(r"\b" + name + r":\[([01,]+)\]", t)
    return [int(x) for x in m.group(1).split(",")] if m else None


def reads(t, r):
    """does instruction t read VGPR r?  A source pair of a packed fp32 instruction is read per half: the low lane takes the half op_sel
    names (default low), the high lane the half op_sel_hi names (default high)"""
    op, ops = t.split()[0], operands(t)
    if ALL_READS.match(op):
        return any(r in vregs(o) for o in ops)
    if READS_DEST.search(op) and r in vregs(ops[0]):
        return True
    if PK_FLOAT.match(op):
        sel, sel_hi = modifier(t, "op_sel", 3) or [0, 0, 0], modifier(t, "op_sel_hi", 3) or [1, 1, 1]
        for k, o in enumerate(ops[1:]):
            v = vregs(o)
            if len(v) == 2 and r in v:
                if {sel[k], sel_hi[k]} & {v.index(r)}:
                    return True
            elif r in v:
                return True
        return False
    return any(r in vregs(o) for o in ops[1:])


def live_after(ins, i, r):
    """is the value instruction i leaves in VGPR r read on any path before it is overwritten?  (walks the branches of the kernel's own
    labels; a register still unread at s_endpgm is dead)"""
    at = {t[:-1]: j for j, t in enumerate(ins) if t.endswith(":")}
    seen, stack = set(), [i + 1]
    while stack:
        j = stack.pop()
        while j < len(ins) and j not in seen:
            seen.add(j)
            t = ins[j]
            if t.endswith(":"):
                j += 1
                continue
            if reads(t, r):
                return True
            op = t.split()[0]
            if op == "s_endpgm" or (not ALL_READS.match(op) and r in vregs(operands(t)[0])):
                break
            m = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)$", t)
            if m and op == "s_branch":
                j = at[m.group(1)]
                continue
            if m:
                stack.append(at[m.group(1)])
            j += 1
    return False


def float_ops(ins):
    """multiset of the floating-point opcodes: what decides, next to the order of the sums, whether results can differ by a bit (hipcc
    contracts a * b + c where it finds both in one basic block, so moving code can change which products are fused).  v_fmac is v_fma
    with the addend in the destination.  A packed instruction is two scalar ones -- or one, where the other half of its result is
    never read (hipcc emits such a v_pk_fma_f32 for a scalar fma whose operands sit in register pairs)."""
    out = collections.Counter()
    for i, t in enumerate(ins):
        if FLOAT_OPS.match(t):                    # encodings (_e32, _e64, _dpp) do not matter
            op = re.sub(r"_(e32|e64|dpp|sdwa)$", "", t.split()[0])
            n = 1
            if op.startswith("v_pk_"):
                n = 2
                if PK_FLOAT.match(op):
                    n = max(1, sum(live_after(ins, i, r) for r in vregs(operands(t)[0])))
            out[op.replace("v_pk_", "v_").replace("v_fmac_", "v_fma_")] += n
    return out


def hot_loops(ins):
    """innermost backward-branch loops that hold MFMAs, labels stripped"""
    at = {t[:-1]: i for i, t in enumerate(ins) if t.endswith(":")}
    spans = []
    for i, t in enumerate(ins):
        m = re.match(r"s_cbranch\S*\s+(\.LBB\d+_\d+)$", t) or re.match(r"s_branch\s+(\.LBB\d+_\d+)$", t)
        if m and at.get(m.group(1), i) < i:
            spans.append((at[m.group(1)], i))
    inner = [s for s in spans if not any(o != s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]
    out = []
    for a, b in inner:
        body = [re.sub(r"\.LBB\d+_\d+", ".L", t) for t in ins[a + 1:b + 1] if not t.endswith(":")]
        if any(t.startswith("v_mfma") for t in body):
            out.append(body)
    return out


def main_loop(ins):
    ins = [t for t in ins if not t.endswith(":")]
    at = [i for i, t in enumerate(ins) if t.startswith("v_mfma")]
    return ins[at[0]:at[-1] + 1] if at else []


def unreg(t):
    return re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", t)


def loop_class(a, b):
    if a == b:
        return "identical"
    if [unreg(t) for t in a] == [unreg(t) for t in b]:
        return "identical up to register numbers"
    oa, ob = [t.split()[0] for t in a], [t.split()[0] for t in b]
    if oa == ob:
        return "the same opcode sequence"
    ca, cb = collections.Counter(oa), collections.Counter(ob)
    if ca == cb:
        return f"NONE: the same opcode multiset in another order ({len(oa)} instructions)"
    diff = {k: cb[k] - ca[k] for k in set(ca) | set(cb) if ca[k] != cb[k]}
    return f"NONE: {len(oa)} -> {len(ob)} instructions, opcode counts new - parent: {dict(sorted(diff.items()))}"


def main(ps, pr, ns, nr):
    kp, kn, rp, rn = kernels(ps), kernels(ns), resources(pr), resources(nr)
    names = sorted(kp)
    pretty = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")))
    short = {k: re.sub(r"\(.*", "", pretty[k].replace("void ", "")) for k in names}
    ok = sorted(kn) == names
    print(f"kernels: parent {len(kp)}, new {len(kn)}, the same names: {ok}")
    if not ok:
        print("  only in parent:", sorted(set(kp) - set(kn)), " only in new:", sorted(set(kn) - set(kp)))
        names = sorted(set(kp) & set(kn))
    cols = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "LDS", "Occupancy")
    print("kernel | body | main loop (first to last v_mfma) ; per build: " + " ".join(cols) + " instr " + " ".join(COUNTED))
    nsame = 0
    for k in names:
        ia, ib = instrs(kp[k]), instrs(kn[k])
        a, b, sa, sb = rp[k], rn[k], stats(ia), stats(ib)
        cond = (b["ScratchSize"] <= a["ScratchSize"] and b["Occupancy"] >= a["Occupancy"] and b["LDS"] <= a["LDS"]
                and all(sa[c] == sb[c] for c in COUNTED))
        ok = ok and cond
        same = kp[k] == kn[k]
        nsame += same
        fa, fb = float_ops(ia), float_ops(ib)
        if fa != fb:
            ok = False
            print(f"  {short[k]:58s} FLOAT OPCODES DIFFER, new - parent: { {o: fb[o] - fa[o] for o in sorted(set(fa) | set(fb)) if fa[o] != fb[o]} }")
        print(f"  {short[k]:58s} | {'byte-identical' if same else 'differs       '} | {loop_class(main_loop(ia), main_loop(ib))}{'' if cond else '   CONDITION BROKEN'}")
        la, lb = hot_loops(ia), hot_loops(ib)
        if not same:
            if len(la) != len(lb):
                print(f"  {'':58s}   inner MFMA loops: parent {len(la)}, new {len(lb)}")
            for n, (x, y) in enumerate(zip(la, lb)):
                print(f"  {'':58s}   inner loop {n} ({sum(t.startswith('v_mfma') for t in x)} MFMAs): {loop_class(x, y)}")
        fmt = lambda r, s: " ".join(f"{r[c]:6d}" for c in cols) + f" {s['lines']:6d} " + " ".join(f"{s[c]:4d}" for c in COUNTED)
        if not same or not cond:
            print(f"  {'':58s}   parent {fmt(a, sa)}\n  {'':58s}   new    {fmt(b, sb)}")
    print(f"{nsame} of {len(names)} kernel bodies byte-identical")
    print("same names, scratch <= parent, waves per SIMD >= parent, LDS <= parent, counted instructions and floating-point opcode counts equal:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:5]))
