"""Launch times of the attention prologue at the bench's shapes, one build per process (profiles/qkv_shared_parts.txt, step 5).

  [ONIRIS_LIB_NAME=<build>] python scratch/qkv_parts_kernels.py [REPS] > DIR/<build>_kernels_<i>.json

qkv_norm_rope_kernel and qkv_norm_rope_bwd_kernel on the gym net's VideoAttention layer in training (B = 8 sequences, 2 x 64 frames of 64
tokens, 4 heads), oniris_qkv_eval on one new frame of the cached sampler (64 tokens, C = 256, behind 10 committed frames of a 16-frame ring:
qkv_eval_few_kernel).  5 warm-up and REPS timed launches each between two HIP events (ops._timed_launch); one JSON line
{"kernels": {name: {"launches", "us_mean", "us_median"}}}.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from autoregressive_diffusion_amd import ops

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
lib, p, st = ops.lib, ops._p, ops._stream
torch.manual_seed(0)
inv = (1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))).cuda()
scv = ((torch.arange(0, 64, 2) + 0.4 * 64) / (1.4 * 64)).cuda()
bf = dict(device="cuda", dtype=torch.bfloat16)

B, T, P, C = 8, 64, 64, 256
ntok = B * 2 * T * P
cs, sn, sc = [t.contiguous() for t in ops.rope_tables(inv, scv, T, "cuda")]
qkv = torch.randn(ntok, 3 * C, **bf)
q, k, v, dqkv = torch.empty(ntok, C, **bf), torch.empty(ntok, C, **bf), torch.empty(ntok, C, **bf), torch.empty(ntok, 3 * C, **bf)
dq, dk, dv = torch.randn(ntok, C, **bf), torch.randn(ntok, C, **bf), torch.randn(ntok, C, **bf)

cap, n = 16, 10
ecs, esn, esc = [t.contiguous() for t in ops.rope_tables(inv, scv, n + 1, "cuda")]
x, w = torch.randn(P, C, **bf), (torch.randn(3 * C, C, device="cuda") / 16).to(torch.bfloat16)
eq, ek, ev, ekr = torch.empty(P, C, **bf), torch.zeros(cap * P * C, **bf), torch.zeros(cap * P * C, **bf), torch.zeros(cap * P * C, **bf)

LAUNCHES = {
    "qkv_norm_rope_kernel": lambda: ops.check(lib.oniris_qkv_norm_rope(p(qkv), p(q), p(k), p(v), p(cs), p(sn), p(sc), ntok, C, P, T, st()), "qkv_norm_rope"),
    "qkv_norm_rope_bwd_kernel": lambda: ops.check(lib.oniris_qkv_norm_rope_bwd(p(qkv), p(dq), p(dk), p(dv), p(dqkv), p(cs), p(sn), p(sc), ntok, C, P, T,
                                                                              st()), "qkv_norm_rope_bwd"),
    "oniris_qkv_eval": lambda: ops.check(lib.oniris_qkv_eval(p(x), p(w), p(eq), p(ek), p(ev), p(ekr), p(ecs), p(esn), p(esc), P, C, C, P, cap * P * C,
                                                             n * P, n, st()), "qkv_eval"),
}
out = {}
for name, fn in LAUNCHES.items():
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ev_ = [ops._timed_launch(fn) for _ in range(reps)]
    torch.cuda.synchronize()
    us = [1e3 * a.elapsed_time(b) for a, b in ev_]
    out[name] = dict(launches=reps, us_mean=round(statistics.mean(us), 3), us_median=round(statistics.median(us), 3))
print(json.dumps({"kernels": out}))
