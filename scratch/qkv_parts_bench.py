"""Speed of two builds, alternating within one call (profiles/qkv_shared_parts.txt, step 5).

  per run i of a build (parent: ONIRIS_LIB_NAME=<parent build>), builds alternating, at least three runs each:
    python bench.py --gpus 1 --steps 20 --warmup 5                                  > DIR/<build>_bench_<i>.json     (the headline)
    python bench.py --mode rollout --batch 1 --gen-frames 256 --ctx-frames 8        > DIR/<build>_rollout_<i>.json   (what extra.rollout_256 runs)
    python scratch/qkv_parts_kernels.py                                             > DIR/<build>_kernels_<i>.json
  python scratch/qkv_parts_bench.py DIR

The margin is the parent's own spread: the new build's median must lie within the range the parent's runs span, or on the better side of it.
"""
import glob
import json
import os
import statistics
import sys


def load(d, build, what):
    runs = []
    for path in sorted(glob.glob(os.path.join(d, f"{build}_{what}_*.json"))):
        runs.append(json.loads([l for l in open(path) if l.startswith("{")][-1]))
    return runs


def line(name, p, n, higher_is_better):
    med = statistics.median(n)
    good = med >= min(p) if higher_is_better else med <= max(p)
    inside = min(p) <= med <= max(p)
    print(f"  {name:36s} | parent {min(p):10.3f} .. {max(p):10.3f} median {statistics.median(p):10.3f} | new {min(n):10.3f} .. {max(n):10.3f} "
          f"median {med:10.3f} | median new / parent {med / statistics.median(p):.4f}  "
          f"{'inside the range of the parent' if inside else 'better than the range of the parent' if good else 'OUTSIDE THE RANGE OF THE PARENT'}")
    return good


def main(d):
    ok = True
    for what, name, hib in (("bench", "headline latent-frames/s", True), ("rollout", "rollout_256 frames/s", True)):
        p, n = [r["value"] for r in load(d, "parent", what)], [r["value"] for r in load(d, "new", what)]
        print(f"{what}: runs parent {len(p)}, new {len(n)}")
        ok = len(p) >= 3 and len(n) >= 3 and line(name, p, n, hib) and ok
    p, n = load(d, "parent", "bench"), load(d, "new", "bench")
    print("  loss of the last step  parent", sorted({r["loss"] for r in p}), " new", sorted({r["loss"] for r in n}))
    p, n = load(d, "parent", "kernels"), load(d, "new", "kernels")
    print(f"kernels: runs parent {len(p)}, new {len(n)}; us per launch, median of {p[0]['kernels']['oniris_qkv_eval']['launches']} launches per run")
    for k in p[0]["kernels"]:
        ok = line(k, [r["kernels"][k]["us_median"] for r in p], [r["kernels"][k]["us_median"] for r in n], False) and ok
    print("the median of the new build inside the parent's range or better, everywhere:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
