"""The shapes and inputs of the step-edge kernel tests  --  TEST INFRASTRUCTURE shared by tests/test_step_edge_gpu.py (the kernels) and
tests/test_step_edge_oracle.py (which evaluates the restatements in float32 on these very inputs).  CPU tensors, seeded.
Every frame, layer and row gets its own sigma, gain or label, so that a wrong index lands on a different value; sigmas are
log-uniform over the EDM range 0.002 ... 80 with both ends present (a case with a single sigma takes the end named there)."""
import math

import torch

BF16 = torch.bfloat16
NAN = float("nan")
SD = 0.5                  # sigma_data
SIG_LO, SIG_HI = 0.002, 80.0


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def floored(g, *shape, lo=0.5, hi=1.0):
    """Random signs times magnitudes in [lo, hi]: no element is small."""
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return sign * (lo + (hi - lo) * torch.rand(*shape, generator=g))


def sigmas(g, *shape, single=SIG_LO):
    s = torch.exp(math.log(SIG_LO) + (math.log(SIG_HI) - math.log(SIG_LO)) * torch.rand(*shape, generator=g))
    flat = s.reshape(-1)
    flat[0] = single
    if flat.numel() > 1:
        flat[0], flat[-1] = SIG_LO, SIG_HI
    return s.float()


# (B, S, T, C, H, W, cpad)
DART_INPUT = [(2, 2, 3, 4, 5, 7, 32),        # HW = 35: one ragged block
              (1, 2, 1, 8, 16, 20, 32),      # HW = 320: a ragged second block
              (1, 1, 2, 15, 8, 8, 16),       # C = 15 (the ones channel is the last of the 16 the kernel builds), S = 1, cpad = 16
              (1, 2, 2, 1, 3, 3, 64),        # C = 1, cpad = 64: six zero vectors behind the first two
              (1, 1, 1, 3, 130, 127, 32)]    # HW = 16510 > 64 * 256: the grid cap, a second trip of the pixel loop (one sigma: 0.002)


def dart_input_inputs(case):
    B, S, T, C, H, W, cpad = case
    g = gen(100 + C + H)
    return rn(g, B, T, C, H, W), rn(g, B, S * T, C, H, W), sigmas(g, B, S * T)


# (B, T, C, H, W)
DART_PAIR = [(2, 3, 4, 5, 7), (1, 1, 8, 16, 20)]       # the second: one source row, rows 0 and 1 both pack it (sigma 0.002)


def dart_pair_inputs(case):
    B, T, C, H, W = case
    g = gen(150 + C)
    return rn(g, B, T, C, H, W, scale=3.0), sigmas(g, B, T)


# (B, S, T, C, H, W)
DART_LOSS = [(2, 2, 3, 4, 5, 7),             # HW = 35: most of the 1024 threads idle
             (1, 2, 2, 8, 33, 32),           # HW = 1056: the second pass of `p += blockDim.x` is ragged (32 threads)
             (1, 1, 2, 3, 64, 64),           # HW = 4096 (the gym step's): four passes; S = 1: no clean slots
             (2, 2, 1, 1, 16, 16)]           # T = 1, C = 1


def dart_loss_inputs(case):
    """F's pad channels c >= C hold NaN: no output may see them.  dlosses is distinct per frame."""
    B, S, T, C, H, W = case
    g = gen(200 + C + H)
    F = rn(g, B * S * T, H, W, 8).to(BF16)
    F[..., C:] = NAN
    dl = floored(g, B, T) * (1 + torch.arange(B * T).reshape(B, T))
    return F, rn(g, B, T, C, H, W), rn(g, B, S * T, C, H, W), sigmas(g, B, S * T), dl


# (B, T, S, nterms, cap, starting count)
LOSS_TAIL = [(8, 64, 2, 4, 10000, 0),              # n = 512 > 256 threads: two entries per thread (the gym step's)
             (3, 5, 1, 1, 7, 5),                   # n = 15 > cap = 7: only the last 7 are logged, slots wrap; nterms = 1: m = 10^(c0/2)
             (2, 64, 2, 4, 300, 2 ** 31 + 3)]      # a history count beyond 2^31: the slot arithmetic is 64-bit


def loss_tail_inputs(case):
    B, T, S, nterms, cap, count = case
    g = gen(300 + T + cap)
    mse = torch.rand(B, T, generator=g) + 0.1
    coef = rn(g, 2 * nterms - 1, scale=0.3)
    rings = (-1.0 - torch.arange(cap).float(), -2.0 - torch.arange(cap).float(), -3 - torch.arange(cap, dtype=torch.int32))
    return mse, sigmas(g, B, S * T), coef, rings


# (N, C, H, W)
PRECOND = [(3, 4, 5, 7), (2, 8, 16, 20),
           (1, 3, 130, 127),                 # HW = 16510 > 64 * 256: the grid cap (one sigma: 80)
           (4, 1, 8, 8)]
GUIDANCE = [0.0, 0.3, -0.3, 0.5, 1.0, 1.7, -2.0]       # |g| < 0.5 | at 0.5 | beyond 1 | negative


def precond_inputs(case):
    """F (2N, HW, 8): rows [0, N) the 3-D half, [N, 2N) the 2-D half; pad channels NaN.  x at the scale sqrt(sigma^2 + sd^2) the
    sampler's x has, so that c_skip x and c_out F are both O(1) at either end of the sigma range."""
    N, C, H, W = case
    g = gen(400 + C + H)
    F = rn(g, 2 * N, H * W, 8).to(BF16)
    F[..., C:] = NAN
    sg = sigmas(g, N, single=SIG_HI)
    x = rn(g, N, C, H * W) * (sg * sg + SD * SD).sqrt().reshape(N, 1, 1)
    return F, x, sg


# (L, N, T)
GATES = [(5, 6, 3),
         (3, 1024, 64),                      # the gym step's: four passes of gates_bwd's loop
         (2, 294, 7),                        # N ragged against the 256-thread block
         (1, 16390, 5)]                      # > 64 * 256: the grid cap of gates; gates_bwd: 65 passes per thread (chain 65 + 6 + 2 = 73)
NCTX = ["null", "mixed", "1000"]


def gates_inputs(case, nctx_kind, saturated=False):
    L, N, T = case
    g = gen(500 + N)
    c_noise = sigmas(g, N).log() / 4
    params = rn(g, L, 6, scale=0.7) + torch.tensor([1.5, -0.5, 0, 0, -1.0, 1.0])
    if saturated:                             # sv ~ +-60 through off0; min_gating, max_gating ~ +-30
        assert L == 4
        params[0, 2], params[1, 2] = 60.0, -60.0
        params[2, 4], params[2, 5] = 30.0, -30.0
        params[3, 4], params[3, 5] = -30.0, 30.0
    nctx = {"null": None, "mixed": (torch.arange(L, dtype=torch.int32) * 7 + 3) % 11, "1000": torch.full((L,), 1000, dtype=torch.int32)}[nctx_kind]
    return c_noise, params, nctx, rn(g, L, N), rn(g, L, N)


# (N, cn, cemb, L)
EMBED_EVAL = [(6, 16, 64, 4),
              (3, 512, 300, 1),              # cn at its limit (the shared array's 512); a ragged second pass of `co += 256`
              (2, 12, 520, 5)]               # three passes
LABELS = ["none", "no-weight", "in-range", "L", "-1"]


def embed_eval_inputs(case, label_kind):
    """Row 1 of w_noise is all zero: e = 0 / 1e-4 = 0 there.  'in-range' labels include L - 1; 'L' and '-1' are out of range."""
    N, cn, cemb, L = case
    g = gen(600 + cn)
    c_noise = sigmas(g, N).log() / 4
    freqs, phases = 2 * math.pi * rn(g, cn), 2 * math.pi * torch.rand(cn, generator=g)
    w_noise, w_label = rn(g, cemb, cn), rn(g, cemb, L)
    w_noise[1] = 0
    labels = {"none": None, "no-weight": (torch.arange(N) + L - 1) % L, "in-range": (torch.arange(N) + L - 1) % L,
              "L": torch.full((N,), L), "-1": torch.full((N,), -1)}[label_kind]
    return c_noise, labels, freqs, phases, w_noise, (None if label_kind == "no-weight" else w_label)


# (N, cn, cnP, L, LP)
EMBED_PRE = [(6, 12, 16, 4, 8), (2, 5, 8, 9, 16), (3, 512, 512, None, None),
             (4, 7, 8, 5, 8)]               # sqrt(5) is no bf16 value: the one-hot entry is a ROUNDED float32 square root (2.234375)


def embed_pre_inputs(case):
    N, cn, cnP, L, LP = case
    g = gen(700 + cn)
    c_noise = sigmas(g, N).log() / 4
    labels = (torch.arange(N) * 3 + L - 1) % L if L else None
    return c_noise, labels, 2 * math.pi * rn(g, cn), 2 * math.pi * torch.rand(cn, generator=g)


EMBED_POST_N = [384, 262221]                 # 262221 > 1024 * 256: the block cap, a ragged second trip
EMBED_POST_T = [1 / 3, 0.5, None]            # None: e2 = NULL


def embed_post_inputs(n, t):
    """|e| <= 8, and a few elements at +-40 (sigmoid saturated either way)."""
    g = gen(800 + n)
    e1, e2, demb = (rn(g, n, scale=2.5).clamp(-8, 8).to(BF16) for _ in range(3))
    e1[3], e1[n - 2], e2[3], e2[n - 2], e2[7] = 40.0, -40.0, 40.0, -40.0, -40.0
    return e1, (None if t is None else e2), demb


# (N, widths)
EMB_SCALE = [(7, [64, 128, 64]),
             (1024, [64, 128]),              # the gym step's N: 64 rows per chunk, chain 32 + 6 + 2
             (5, [40, 8, 72]),               # ragged widths; N < 16: eleven empty row chunks, whose dgain_part must be written 0
             (33, [64])]                     # K = 1; chunks of 2 and 3 rows


def emb_scale_inputs(case, exact=False):
    N, widths = case
    g = gen(900 + N)
    Ct, K = sum(widths), len(widths)
    seg = torch.tensor([k for k, w in enumerate(widths) for _ in range(w)], dtype=torch.int32)
    start = torch.tensor([sum(widths[:k]) for k in range(K + 1)], dtype=torch.int32)
    if exact:                                 # small integers and power-of-two gains: every product and partial sum is exact
        c_all = torch.randint(-4, 5, (N, Ct), generator=g).to(BF16)
        gain = 2.0 ** torch.randint(-1, 2, (K,), generator=g).float() * (torch.arange(K) % 2 * 2 - 1)
        dc = torch.randint(-4, 5, (N, Ct), generator=g).float()
    else:
        c_all, gain, dc = rn(g, N, Ct).to(BF16), floored(g, K) * (1 + torch.arange(K)), rn(g, N, Ct)
    return c_all, gain, seg, start, dc
