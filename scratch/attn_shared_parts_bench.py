"""Speed of two builds on the flagship workload, alternating (profiles/attn_shared_parts.txt, step 5).

  ONIRIS_LIB_NAME=<parent build> python bench.py --gpus 1 --steps 20 --warmup 5 --full --no-extra --cpu-frames 0  > DIR/parent_<i>.json
  python bench.py --gpus 1 --steps 20 --warmup 5 --full --no-extra --cpu-frames 0                                  > DIR/new_<i>.json     (i = 1..6, alternating)
  python scratch/attn_shared_parts_bench.py DIR

The margin is the parent's own run-to-run range: the headline (latent-frames/s, higher is better) and ms_total of every attention key of
the profiled cycle (lower is better) of every new run must lie inside the parent's range or on the better side of it.
"""
import glob
import json
import os
import sys

ATTN = ("attn", "qkv_norm", "rope")


def load(pattern):
    runs = []
    for path in sorted(glob.glob(pattern)):
        line = [l for l in open(path) if l.startswith("{")][-1]
        runs.append(json.loads(line))
    return runs


def main(d):
    parent, new = load(os.path.join(d, "parent_*.json")), load(os.path.join(d, "new_*.json"))
    print(f"runs: parent {len(parent)}, new {len(new)}")
    ok = len(parent) >= 6 and len(new) >= 6
    pv, nv = [r["value"] for r in parent], [r["value"] for r in new]
    good = min(nv) >= min(pv)
    ok = ok and good
    if max(pv) > 0:          # (the runs of attn_shared_parts_kernels.py carry no headline)
        print(f"headline latent-frames/s  parent {min(pv):.2f} .. {max(pv):.2f}  new {min(nv):.2f} .. {max(nv):.2f}  {'inside / better' if good else 'BELOW THE RANGE'}")
    print("loss  parent", sorted({r['loss'] for r in parent}), " new", sorted({r['loss'] for r in new}))
    keys = sorted(k for k in parent[0]["kernels"] if any(a in k for a in ATTN))
    print("attention keys of the profiled cycle, ms_total (launches): parent range | new range")
    for k in keys:
        p = [r["kernels"][k]["ms_total"] for r in parent if k in r["kernels"]]
        n = [r["kernels"][k]["ms_total"] for r in new if k in r["kernels"]]
        good = bool(n) and max(n) <= max(p)
        ok = ok and good
        print(f"  {k:64s} ({parent[0]['kernels'][k]['launches']:4d})  {min(p):8.3f} .. {max(p):8.3f} | {min(n):8.3f} .. {max(n):8.3f}  {'inside / better' if good else 'ABOVE THE RANGE'}")
    missing = sorted(set(keys) ^ set(k for k in new[0]["kernels"] if any(a in k for a in ATTN)))
    print("keys in one build only:", missing)
    print("every new run inside the parent's range or better:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
