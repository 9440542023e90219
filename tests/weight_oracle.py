"""Float64 restatements of the weight and optimizer kernels (upper half of csrc/weights.hip: weight_prep_kernel, weight_wb_kernel,
weight_bwd_kernel, adamw_kernel, sqnorm_partial_kernel / sqnorm_final_kernel)  --  TEST INFRASTRUCTURE.  One function per kernel,
written as a function of exactly what that kernel reads (fp32 parameters, bf16 slabs, the fp32 values of the hyper-parameters, the
squared gradient norm the kernel found in its scratch), plain CPU tensors in, float64 out.

Every result is a pair (value, mag): `mag` is the same expression with every addend replaced by its absolute value, as in
glue_oracle.py, whose constants the bounds are made of (u = 2^-24, one fp32 unit roundoff):

  wf, wb                       |got - value| <= 2^-8 |value| + 2^-18 mag   (bound_bf16: one bf16 rounding + 64 u)
  w_new, m, v, p, EMA copies   |got - value| <= 2^-18 mag                  (U_F32_64: 64 u, fp32 elementwise)
  grad, sqnorm on Gaussians    |got - value| <= 2^-17 mag                  (bound_f32: 128 u, fp32 reductions)
  exact                        padding (bit-zero), everything "untouched" (eval parameters, identity rows, p / m / v at step 0, .grad
                               at nsplit = 0, g, guards), wb against the transpose of the kernel's own bf16 wf, and sqnorm on
                               ternary data whose count stays below 2^24 (every partial sum is an integer fp32 holds)

Why 64 u cover the elementwise results.  w_new = w / den, den = eps + sqrt(ss) / sqrt(fan): ss is a sum of fan positive terms
whose longest chain of additions is ceil(fan / 256) per thread (each one fused with its product) + 6 butterfly steps + 3 additions
of the four waves' sums; the square root halves the relative error.  Per weight of tests/test_weight_stages_gpu.py:
    fan    16   24   72   45  5184  5760   64  1440   64  288  256 (identity rule)
    chain  10   10   10   10    30    32   10    15   10   11   10        -> at most 16 u on sqrt(ss)
plus sqrt, the hardware rsqrt of fan (1 ulp = 2 u) and its product, the addition of eps, the reciprocal (1 ulp) and the final
product: <= 8 u.  w_new: <= 24 u.  wf = w_new * scale carries the second normalisation as well (another <= 24 u, gain and one more
product) -- 50 u by this count, under 64; a common relative error of the row's w_new cancels in w_new * scale, so the sum
overstates it.  eps itself is the fp32 1e-4f in the kernel (pass eps = EPS_F32): against 1e-4 it moves den by 2.5e-12.
The identity rule (|den - 1| < 4e-7 leaves the row alone) is decided here in float64.  Where fp32 decides otherwise the two answers
differ by |den - 1| |w| / den < (4e-7 + 4.2e-7) |w| = 14 u |w| (the second figure: how far the fp32 den can be from the float64
one at fan <= 256, see test_identity_rule), inside the bound; test_identity_rule itself uses rows away from the edge.

adamw: at most 6 operations behind m and v, about 16 behind p (m, v, two divisions, sqrt, + eps, division, two products, the
subtraction, lr * wd and 1 - lr * wd) and 3 more behind an EMA copy: under 32 u.  The bias corrections come from the host as fp32
1 - powf(beta, step); the restatement uses the exact power of the fp32 beta.  powf is good to 1 ulp of beta^step (<= 2 u beta^step),
so bc is off by at most (2 beta^step + 1) u / (1 - beta^step) relatively: 0 at step 1 (powf(b, 1) = b and 1 - b is exact for
b in [1/2, 1]), largest at small steps > 1.  At the steps and betas of the GPU tests:
    step 3:     beta1 = 0.9: 9 u;   beta2 = 0.99: 99 u on bc2, halved by the square root: 50 u;   beta1 = 0.8: 4 u;  beta2 = 0.95: 19 u / 2
    step 1000:  beta^step < 5e-5 (0.99), 0 for the others: 1 u
These act on the update term lr * mh / (sqrt(vh) + eps) alone.  Where |p| ~ 1 that term is a small part of mag(p), but on an
element with p near 0 it is all of it, and there the 1-ulp figure (9 + 50 u, on top of 16 operations) would NOT fit into 64 u: the
derivation needs what powf really does.  test_powf_error_is_covered calls the C library's powf -- the host's -- at every (beta, step)
of the GPU tests and asserts that bc1's error plus half of bc2's is at most 16 u (measured: 1.8 + 12.7 / 2 u at 0.9 / 0.99, step 3),
which with the 16 operations leaves half of the bound unused even where p = 0.
`gnorm_sq` is the value the kernel read, so the reduction's error stays out of the elementwise bound; near coef = 1 both
decisions give the same factor to 1 u.

Why 128 u cover the reductions.  weight_bwd: G is the sum of nsplit slabs over four accumulators (<= ceil(19 / 4) + 2 = 7
additions; exact on the integer slabs), dot = <G, w> and |w|^2 have the chain ceil(fan / 256) + 6 + 3 of the table above (<= 32),
k1 and k2 cost <= 10 operations, the result three more: <= 7 + 32 + 13 = 52 u on the worst element, measured against
|grad0| + k1 sum_s |slab_s| + k2' |w|, where k2' is k2 with sum |G w| in place of dot.  sqnorm: 4 additions per trip and thread
(n <= 2 * 2^20 + 1203: 3 trips = 12), 6 + 3 in the block, then <= 4 + 6 + 3 over the block partials: <= 34 u.

tests/test_weight_oracle.py pins every function to oracle.oniris_oracle.weight_effective, float64 autograd and torch's own
clip_grad_norm_ / AdamW / lerp_, and checks that the bounds are neither too tight nor too loose.  `dtype = torch.float32` evaluates
the same formulas in float32 with the sums in the kernels' order (per-thread strides of 256, butterfly, waves) for that review."""
import ctypes
import ctypes.util
import math
import types

import torch

import glue_oracle as GO

EPS = 1e-4
EPS_F32 = float(torch.tensor(1e-4, dtype=torch.float32))           # W_EPS as the kernels read it
CLIP_EPS = 1e-6
CLIP_EPS_F32 = float(torch.tensor(1e-6, dtype=torch.float32))
IDENT = 4e-7                                                       # weight_prep_kernel's identity threshold on |den - 1|
F64, F32 = torch.float64, torch.float32
bound_bf16, bound_f32, U_F32_64 = GO.bound_bf16, GO.bound_f32, GO.U_F32_64       # the bounds are glue_oracle's, unchanged


def f32(x):
    """The fp32 value a kernel receives for a host double."""
    return float(torch.tensor(x, dtype=F32))


def roundup(a, b):
    return -(-a // b) * b


def perm_rows(cout, perm3):
    """Packed row of every output channel: qkv rows (m c s) -> (s m c)."""
    co = torch.arange(cout)
    return (co % 3) * (cout // 3) + co // 3 if perm3 else co


def flipped_taps(taps, kt):
    """wb's tap for every wf tap: flipped spatially within its temporal slice."""
    per_t = taps // kt
    t = torch.arange(taps)
    j, k = t // per_t, t % per_t
    return j * per_t + (per_t - 1 - k)


def _geom(w):
    cout, cin = w.shape[:2]
    taps = math.prod(w.shape[2:]) if w.ndim > 2 else 1
    return cout, cin, taps


def _block_sum32(part):
    """common.h block_sum on (rows, 256) float32 per-thread values: xor butterfly over the 64 lanes, then the four waves in order."""
    x = part.reshape(-1, 4, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lane ^ o]
    return ((x[:, 0, 0] + x[:, 1, 0]) + x[:, 2, 0]) + x[:, 3, 0]


def _rowsum(x, dtype):
    """Sum over the last axis of (rows, n).  float64: plain.  float32: thread t adds elements t, t + 256, ... in order, then block_sum."""
    if dtype == F64:
        return x.sum(-1)
    rows, n = x.shape
    k = -(-n // 256)
    pad = torch.zeros(rows, k * 256, dtype=x.dtype)
    pad[:, :n] = x
    pad = pad.reshape(rows, k, 256)
    acc = pad[:, 0].clone()
    for i in range(1, k):
        acc = acc + pad[:, i]
    return _block_sum32(acc)


def _scalar(x, dtype):
    return torch.tensor(x, dtype=dtype)


def _pow(b, step):
    """b^step.  float32: the C library's powf, which is what the host calls for the bias corrections (torch's pow without it)."""
    if b.dtype == F64:
        return b ** step
    try:
        libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        libm.powf.restype, libm.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
        return torch.tensor(libm.powf(float(b), float(step)), dtype=F32)
    except (OSError, AttributeError):
        return b ** step


# ---------------------------------------------------------------------------------------------------------------------
def row_den(w, eps=EPS, dtype=F64):
    """den = eps + |w_row| / sqrt(fan) of every output row: what weight_prep_kernel divides by in training mode."""
    cout, cin, taps = _geom(w)
    W = w.detach().to("cpu", dtype).reshape(cout, cin * taps)
    return eps + _rowsum(W * W, dtype).sqrt() * _scalar(float(cin * taps), dtype).rsqrt()


def prep(w, gain, training, perm3=False, kt=1, goff=0, rows=None, eps=EPS, dtype=F64, defect=None):
    """weight_prep_kernel + weight_wb_kernel on one weight w (cout, cin, *k).
      training: den = eps + |w_row| / sqrt(fan);  w_new = w / den, or w itself where |den - 1| < 4e-7;  eval: w_new = w
      W = gain / sqrt(fan) * w_new / (eps + |w_new_row| / sqrt(fan))
      wf [taps][CoutP][CinP]:    wf[tap][goff + perm_row(co)][ci] = W[co][ci][tap]
      wb [taps][CoutPb][CinPb]:  wb[j * per_t + (per_t - 1 - k)][ci][goff + perm_row(co)] = W[co][ci][j * per_t + k]
    `goff`, `rows`: the weight is a member of a group (WeightBank.add_group): its rows start at goff of `rows` = Ctot = CoutP = CinPb.
    Returns w_new, wf, wb as (value, mag) pairs over the whole padded images (padding: value 0, mag 0), `identity` (the rows left
    alone) and wf_live / wb_live (the elements that are not padding).
    `defect` (test_weight_oracle): 'no_flip', 'flip_all' (across the temporal slices), 'no_perm' (wf rows in parameter order)."""
    cout, cin, taps = _geom(w)
    fan = cin * taps
    W = w.detach().to("cpu", dtype).reshape(cout, fan)
    rs = _scalar(float(fan), dtype).rsqrt()
    ident = torch.zeros(cout, dtype=torch.bool)
    Wn = W
    if training:
        den = row_den(w, eps, dtype)
        ident = (den - 1).abs() < IDENT
        inv1 = torch.where(ident, torch.ones_like(den), 1 / den)
        Wn = W * inv1[:, None]
    scale = gain * rs / (eps + _rowsum(Wn * Wn, dtype).sqrt() * rs)
    E = (Wn * scale[:, None]).reshape(cout, cin, taps)
    CoutP, CinP = rows or roundup(cout, 32), roundup(cin, 64)
    CoutPb, CinPb = roundup(cin, 32), rows or roundup(cout, 64)
    pr = perm_rows(cout, perm3) + goff
    prf = torch.arange(cout) + goff if defect == "no_perm" else pr
    tb = flipped_taps(taps, kt)
    if defect == "no_flip":
        tb = torch.arange(taps)
    elif defect == "flip_all":
        tb = taps - 1 - torch.arange(taps)
    wf, wb = torch.zeros(taps, CoutP, CinP, dtype=dtype), torch.zeros(taps, CoutPb, CinPb, dtype=dtype)
    wf_live, wb_live = torch.zeros(taps, CoutP, CinP, dtype=torch.bool), torch.zeros(taps, CoutPb, CinPb, dtype=torch.bool)
    wf[:, prf, :cin] = E.permute(2, 0, 1)
    wf_live[:, prf, :cin] = True
    t = torch.zeros(taps, cin, CinPb, dtype=dtype)
    t[:, :, pr] = E.permute(2, 1, 0)
    wb[tb, :cin] = t
    tl = torch.zeros(taps, cin, CinPb, dtype=torch.bool)
    tl[:, :, pr] = True
    wb_live[tb, :cin] = tl
    Wn = Wn.reshape(w.shape)
    return types.SimpleNamespace(w_new=(Wn, Wn.abs()), wf=(wf, wf.abs()), wb=(wb, wb.abs()), identity=ident,
                                 wf_live=wf_live, wb_live=wb_live)


def wb_of(wf_img, cout, cin, kt, CoutPb, CinPb, goff=0):
    """The wb image that belongs to a given bf16 wf image (taps, CoutP, CinP): its transpose tap by tap, flipped -- the same bits,
    no second rounding.  Rows goff ... goff + cout of wf only; zero elsewhere."""
    taps = wf_img.shape[0]
    wb = torch.zeros(taps, CoutPb, CinPb, dtype=wf_img.dtype)
    wb[flipped_taps(taps, kt), :cin, goff:goff + cout] = wf_img[:, goff:goff + cout, :cin].transpose(1, 2)
    return wb


def _slab_sum(S, dtype, four_chain):
    """Sum of the slabs S (ns, ...).  float32: the kernels' four accumulators -- slab s goes to accumulator s % 4 (the four-chain form
    adds its remainder to accumulator 0) -- and (G0 + G1) + (G2 + G3)."""
    if dtype == F64:
        return S.sum(0)
    ns = S.shape[0]
    acc = [torch.zeros_like(S[0]) for _ in range(4)]
    for s in range(ns):
        a = 0 if (four_chain and s >= ns - ns % 4) else s % 4
        acc[a] = acc[a] + S[s]
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


def bwd(w, slabs, nsplit, gain, grad0, perm3=False, goff=0, eps=EPS, dtype=F64, defect=None):
    """weight_bwd_kernel on one weight: w (cout, cin, *k) as the kernel reads it, slabs (>= nsplit, CoutP, taps, CinP) bf16.
      G[co][ci][tap] = sum_{s < nsplit} slabs[s][goff + perm_row(co)][tap][ci]
      n = |w_row|, s = eps + n / sqrt(fan), c = gain / sqrt(fan), k1 = c / s, k2 = c <G, w> / (sqrt(fan) s^2 n)  (0 where n = 0)
      grad = grad0 + k1 G - k2 w                                       (nsplit = 0: grad0)
    mag = |grad0| + k1 sum_s |slab_s| + k2' |w| with sum |G w| in place of <G, w> in k2'.
    `defect`: 'no_perm' (slab row = parameter row), 'drop_slab', 'double_slab', 'no_projection', 'overwrite'."""
    cout, cin, taps = _geom(w)
    fan = cin * taps
    g0 = grad0.detach().to("cpu", dtype).reshape(cout, cin, taps)
    if nsplit <= 0:
        return g0.reshape(w.shape), g0.abs().reshape(w.shape)
    W = w.detach().to("cpu", dtype).reshape(cout, cin, taps)
    pr = (torch.arange(cout) if defect == "no_perm" else perm_rows(cout, perm3)) + goff
    idx = list(range(nsplit))
    if defect == "drop_slab":
        idx.pop(nsplit // 2)
    elif defect == "double_slab":
        idx.append(nsplit // 2)
    S = slabs.detach().cpu()[idx][:, pr][..., :cin].to(dtype).permute(0, 1, 3, 2)          # (ns, cout, cin, taps)
    G, mG = _slab_sum(S, dtype, (cin & 7) != 0 or taps > 27), S.abs().sum(0)
    rs = _scalar(float(fan), dtype).rsqrt()
    GW = (G * W).reshape(cout, fan)
    dot, mdot = _rowsum(GW, dtype), GW.abs().sum(-1)
    n = _rowsum((W * W).reshape(cout, fan), dtype).sqrt()
    s = eps + n * rs
    c = gain * rs
    k1 = c / s
    ok = n > 0
    safe = torch.where(ok, s * s * n, torch.ones_like(n))
    k2 = torch.where(ok, c * dot * rs / safe, torch.zeros_like(n))
    mk2 = torch.where(ok, c * mdot * rs / safe, torch.zeros_like(n))
    if defect == "no_projection":
        k2 = torch.zeros_like(k2)
    if defect == "overwrite":
        g0 = torch.zeros_like(g0)
    k1, k2, mk2 = k1[:, None, None], k2[:, None, None], mk2[:, None, None]
    grad = g0 + k1 * G - k2 * W
    mag = g0.abs() + k1 * mG + mk2 * W.abs()
    return grad.reshape(w.shape), mag.reshape(w.shape)


# ---------------------------------------------------------------------------------------------------------------------
def adamw(p, g, m, v, hyper, step, gscale=1.0, gnorm_sq=None, max_norm=None, emas=(), clip_eps=CLIP_EPS, dtype=F64, defect=None):
    """adamw_kernel.  hyper = (lr, beta1, beta2, eps, weight_decay) and gscale, max_norm, the EMA weights: the fp32 values the kernel
    receives; gnorm_sq: the squared norm the kernel read (None: no clipping); emas = [(copy, 1 - beta), ...].
      coef = max_norm / (sqrt(gnorm_sq) |gscale| + 1e-6);  gr = g * gscale * (coef if coef < 1 else 1)
      m' = b1 m + (1 - b1) gr;  v' = b2 v + (1 - b2) gr^2;  p' = p (1 - lr wd) - lr (m' / bc1) / (sqrt(v' / bc2) + eps),  bc = 1 - b^step
      ema' = ema + w (p' - ema)
    step 0: p, m, v as they are, the EMA copies follow p.  Returns p, m, v and the list of EMA copies as (value, mag) pairs.
    float32: bc1, bc2 from the C library's powf, as the host computes them.
    `defect`: 'swap_bc', 'wd_after', 'clip_always', 'ema_old_p', 'step0_moves'."""
    lr, b1, b2, eps, wd = (_scalar(x, dtype) for x in hyper)
    P, G, M, V = (t.detach().to("cpu", dtype) for t in (p, g, m, v))
    one = _scalar(1.0, dtype)
    if step == 0 and defect != "step0_moves":
        Pn, Mn, Vn = P, M, V
        mP, mM, mV = P.abs(), M.abs(), V.abs()
    else:
        st = max(step, 1)
        gs = _scalar(gscale, dtype)
        if gnorm_sq is not None:
            coef = _scalar(max_norm, dtype) / (_scalar(gnorm_sq, dtype).sqrt() * gs.abs() + _scalar(clip_eps, dtype))
            if bool(coef < 1) or defect == "clip_always":
                gs = gs * coef
        gr = G * gs
        Mn, mM = b1 * M + (one - b1) * gr, (b1 * M).abs() + ((one - b1) * gr).abs()
        Vn, mV = b2 * V + (one - b2) * gr * gr, (b2 * V).abs() + (one - b2) * gr * gr
        bc1, bc2 = one - _pow(b1, st), one - _pow(b2, st)
        if defect == "swap_bc":
            bc1, bc2 = bc2, bc1
        den = (Vn / bc2).sqrt() + eps
        upd, mupd = lr * (Mn / bc1) / den, lr * (mM / bc1) / den
        keep = one - lr * wd
        Pn = (P - upd) * keep if defect == "wd_after" else P * keep - upd
        mP = (P * keep).abs() + mupd
    out = []
    for e, w in emas:
        E, w = e.detach().to("cpu", dtype), _scalar(w, dtype)
        target = P if defect == "ema_old_p" else Pn
        out.append((E + w * (target - E), E.abs() + w * (mP + E.abs())))
    return (Pn, mP), (Mn, mM), (Vn, mV), out


def sqnorm(g, dtype=F64, skip=None):
    """sum(g^2); every addend is positive, mag = value.  float32: the kernels' order -- thread i of <= 1024 blocks of 256 adds
    ((x^2 + y^2) + z^2) + w^2 of its float4 per trip, block_sum, then one block over the block partials.  `skip`: the defect of
    test_weight_oracle, one element left out."""
    x = g.detach().to("cpu", dtype).reshape(-1)
    if skip is not None:
        x = torch.cat([x[:skip], x[skip + 1:]])
    if dtype == F64:
        s = (x * x).sum()
        return s, s.clone()
    n = x.numel()
    nb = max(1, min(1024, (n // 4 + 255) // 256))
    nth = nb * 256
    trips = -(-n // (nth * 4))
    pad = torch.zeros(trips * nth * 4, dtype=dtype)
    pad[:n] = x * x
    pad = pad.reshape(trips, nth, 4)
    acc = torch.zeros(nth, dtype=dtype)
    for t in range(trips):
        q = pad[t]
        acc = acc + (((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3])
    part = _block_sum32(acc.reshape(nb, 256))
    s = _rowsum(part.reshape(1, nb), dtype)[0]
    return s, s.clone()
