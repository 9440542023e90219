"""Compiler output of conv_wgrad.hip in two trees, kernel by kernel (profiles/wgrad_shared_parts.txt, step 1).

  hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Iinclude -Wno-unused-result --cuda-device-only -S -fuse-cuid=none \
        -Rpass-analysis=kernel-resource-usage autoregressive_diffusion_amd/csrc/conv_wgrad.hip -o X.s 2> X.remarks     (in each tree)
  python scratch/wgrad_shared_parts_asm.py PARENT.s PARENT.remarks NEW.s NEW.remarks

Per kernel: byte-identical or not (the text between the kernel's label and its .Lfunc_end, local label numbers left as they are);
for the kernels that differ the resources of both builds and the counts of the instructions the change must not move.  Exit status 1
when a condition of the profile's step 1 does not hold.
"""
import re
import subprocess
import sys

COUNTED = ("v_mfma", "ds_read_b64_tr_b16", "v_cvt_pk_bf16_f32")
EXPECTED = 17


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


def stats(body):
    ins = [l.split()[0] for l in body if l.startswith("\t") and not l.lstrip().startswith((".", ";"))]
    return dict(lines=len(ins), **{c: sum(1 for i in ins if i.startswith(c)) for c in COUNTED})


def main(ps, pr, ns, nr):
    kp, kn, rp, rn = kernels(ps), kernels(ns), resources(pr), resources(nr)
    names = sorted(kp)
    pretty = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")))
    ok = sorted(kn) == names and len(names) == EXPECTED
    print(f"kernels: parent {len(kp)}, new {len(kn)}, the same names: {sorted(kn) == names}")
    same = [k for k in names if kp[k] == kn.get(k)]
    for k in names:
        print(f"  {'byte-identical' if k in same else 'DIFFERS       '}  {pretty[k].replace('void ', '').split('(')[0]}")
    print(f"{len(same)} kernels byte-identical, {len(names) - len(same)} differ")
    cols = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "LDS", "Occupancy")
    print("kernel | per build: " + " ".join(cols) + " instr-lines " + " ".join(COUNTED))
    for k in names:
        a, b, sa, sb = rp[k], rn[k], stats(kp[k]), stats(kn[k])
        cond = (b["ScratchSize"] == 0 and a["ScratchSize"] == 0 and b["Occupancy"] >= a["Occupancy"] and b["LDS"] <= a["LDS"]
                and sa["v_mfma"] == sb["v_mfma"] and sa["ds_read_b64_tr_b16"] == sb["ds_read_b64_tr_b16"])
        ok = ok and cond
        if k in same and cond:
            continue
        fmt = lambda r, s: " ".join(f"{r[c]:6d}" for c in cols) + f" {s['lines']:6d} " + " ".join(f"{s[c]:4d}" for c in COUNTED)
        print(f"  {pretty[k].replace('void ', '').split('(')[0]:44s} | parent {fmt(a, sa)} | new {fmt(b, sb)}{'' if cond else '   CONDITION BROKEN'}")
    print("scratch 0 everywhere, no kernel below its parent in waves per SIMD or above it in LDS, MFMA and transposing-read counts equal:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:5]))
