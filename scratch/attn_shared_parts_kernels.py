"""Launch times of the persistent VideoAttention kernels at the bench shape, one build per process (profiles/attn_shared_parts.txt, step 5).

  [ONIRIS_LIB_NAME=<build>] python scratch/attn_shared_parts_kernels.py [REPS] > DIR/<build>_<i>.json

B = 8 sequences, T = 64 frames of 64 tokens, 4 heads (the gym net's VideoAttention layer in bench.py): 5 warm-up and REPS timed forward +
backward passes under ops.KernelProfile (the launches' own events).  Prints one JSON line {"kernels": {key: {"launches", "ms_total"}}} in
the form scratch/attn_shared_parts_bench.py reads, so that the forward kernel has a figure in every run whether or not it is among the
sixteen longest keys of bench.py's profiled cycle.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from autoregressive_diffusion_amd import ops

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
B, T, P, m = 8, 64, 64, 4
C, N = 64 * m, B * 2 * T
torch.manual_seed(0)
x = torch.randn(N, P, 3 * C, device="cuda").to(torch.bfloat16).requires_grad_(True)
inv = (1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))).cuda()
sc = ((torch.arange(0, 64, 2) + 0.4 * 64) / (1.4 * 64)).cuda()
g = torch.randn(N, P, C, device="cuda").to(torch.bfloat16)
for i in range(5 + reps):
    if i == 5:
        torch.cuda.synchronize()
        ops.KernelProfile.start()
    out = ops.attention_train(x, "video", B, T, m, (inv, sc))
    out.backward(g)
    x.grad = None
agg = ops.KernelProfile.stop()
print(json.dumps({"value": 0.0, "loss": float(out.float().abs().mean()),
                  "kernels": {k: dict(launches=v["launches"], ms_total=round(v["ms"], 4)) for k, v in agg.items()}}))
