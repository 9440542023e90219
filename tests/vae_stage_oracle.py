"""Stage-by-stage oracle of the VAE's training kernels (autoregressive_diffusion_amd/vae_train.py: Res, Down, Up, Out): the cases,
their seeded operands, the float64 and float32 evaluation of the training restatement's own formulas
(tests/vae_train_cpu_restatement.py) under autograd on the CPU, the two metrics and the bounds derived from them, and the
restatement with one deliberate defect at a time.  No kernel is launched here: tests/test_vae_stages_gpu.py runs the kernels
against these functions, tests/test_vae_train.py runs the functions themselves (the comparator against the defects).

Layouts: the oracle is channels-first (B, C, T, H, W) like the reference; the kernels are channels-last.  Every case's loss is
L = sum over its outputs of sum(out_k cos(0.7 i + phi_k)) over the channels-first flat index i (RT.cotangents)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import vae_train_cpu_restatement as RT

OUT_TOL, GRAD_TOL = 1e-5, 5e-5      # the whole-model bounds of tests/test_vae_train_gpu.py: a stage is allowed no more
FACTOR = 5                          # bound = FACTOR x the float32 oracle's own deviation from the float64 oracle (GRAD_TOL's factor)

# ---- the cases.  Res: (B, T, H, W, C, g, emb) -> the (NCH, GPT) it must reach
RES_CASES = {
    "r01": ((1, 1, 5, 7, 3, 1, False), (8, 1)),       # the image inside one tile, odd ragged C, T = g = 1
    "r02": ((2, 4, 16, 17, 8, 2, True), (8, 2)),      # one column into a second tile
    "r03": ((1, 8, 17, 16, 5, 4, True), (8, 4)),      # one row into a second tile row, ragged C
    "r04": ((1, 8, 9, 20, 8, 8, False), (8, 4)),      # g = 8, two thread groups, T = g
    "r05": ((2, 3, 20, 33, 12, 1, True), (16, 1)),    # three tile columns, B > 1
    "r06": ((1, 16, 6, 18, 16, 8, True), (16, 2)),    # four thread groups, T = 2g
    "r07": ((1, 4, 18, 10, 10, 4, False), (16, 2)),   # T = g
    "r08": ((1, 4, 16, 16, 24, 2, True), (32, 1)),    # three weight rows per stage
    "r09": ((1, 8, 7, 19, 32, 8, True), (32, 1)),     # one weight row per stage, eight thread groups
    "r10": ((1, 2, 17, 17, 48, 1, True), (64, 1)),    # ragged, raised LDS limit
    "r11": ((2, 4, 12, 12, 64, 2, False), (64, 1)),   # full width
    "r12": ((1, 8, 6, 6, 64, 8, True), (64, 1)),      # g = 8 at full width, one work item
}
RES_CAP_CASE = ((1, 9, 176, 176, 4, 1, False), (8, 1))   # 121 tiles x 9 frames = 1089 work items on at most 1024 slabs
RES_WRAP_WORK = {"r02": 8, "r05": 36, "r06": 4}          # conv A's work items B (T / g) tiles: all above three slabs

# 1x1 stages: the parameters and the coarse grid (B, T, H, W).  No grid's row count is a multiple of the rows per chunk
# (rpc) of vae_train._lin_dw; d2 and u3 have fewer rows than one chunk.
DOWN_CASES = {                                        # (Cin, tc, sc, C), grid, permuted channels-first view
    "d0": ((3, 1, 1, 12), (2, 3, 5, 7), True),        # as block 0 is fed
    "d1": ((8, 2, 2, 6), (2, 2, 9, 11), False),       # contiguous: the VEC load and the ragged store
    "d2": ((5, 2, 1, 5), (1, 3, 7, 5), False),
    "d3": ((12, 1, 2, 48), (2, 2, 6, 11), False),     # K = Cout: every area window has length 1
    "d4": ((64, 2, 2, 64), (1, 2, 5, 5), False),      # K = 512: 50 rows in chunks of 21
    "d5": ((64, 2, 2, 64), (1, 2, 5, 7), False),      # K = 512: 70 rows, four chunks (d4's 50 rows make three: no wrap on three slabs)
}
UP_CASES = {                                          # (C, tc, sc), grid, permuted view
    "u0": ((5, 2, 2), (2, 3, 5, 7), True),
    "u1": ((12, 2, 1), (1, 3, 9, 17), False),
    "u2": ((24, 1, 2), (2, 2, 5, 9), False),
    "u3": ((8, 1, 1), (1, 1, 3, 5), False),
    "u4": ((64, 2, 2), (1, 2, 5, 7), False),
}
OUT_CASES = {                                         # (C, Cout), grid, the last block (mean | logvar, logvar_multiplier = -1.7)
    "o0": ((8, 16), (2, 3, 7, 11), False),            # 462 rows
    "o1": ((24, 5), (2, 2, 7, 9), False),
    "o2": ((12, 6), (1, 3, 6, 10), True),
    "o3": ((64, 48), (2, 2, 5, 7), False),
}
LIN_WRAP = ("o0", "d5")                               # more than three chunks: these wrap on three slabs


def lin_rpc(K, N):
    """Rows per chunk of the 1x1 weight gradient (vae_train._lin_dw, csrc/vae_train.hip vt_lin_rpc)."""
    return max(8, min(128, 12288 // (K + 1 + N)))


def lin_kn(kind, p):
    """(K, N) of a 1x1 case: the columns of its input and output views."""
    if kind == "down":
        return p[0] * p[1] * p[2] ** 2, p[3]
    if kind == "up":
        return p[0], p[0] * p[1] * p[2] ** 2
    return p


# ---- seeding
def seed_module(module, seed):
    """tests/test_vae_train_gpu.py seed_params (every parameter non-zero) on any parameter holder."""
    from test_vae_train_gpu import seed_params
    return seed_params(module, seed)


def seeded_state_dict(names, shapes, seed):
    """A state dict drawn entry by entry, in the given order, from one generator: logvar_multiplier -1.7; MPFourier's freqs
    2 pi N(0, 1) and phases 2 pi U(0, 1); other vectors 0.1 N(0, 1); conv and linear weights N(0, 1 / fan_in), the t_cond linear
    halved.  The rule of seed_params by name and shape alone, so that fixture G17 stores no parameter."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for name, shape in zip(names, shapes):
        shape = tuple(int(s) for s in shape)
        if name.endswith("logvar_multiplier"):
            v = torch.full(shape, -1.7)
        elif name.endswith(".freqs"):
            v = 2 * math.pi * torch.randn(shape, generator=g)
        elif name.endswith(".phases"):
            v = 2 * math.pi * torch.rand(shape, generator=g)
        elif len(shape) == 1:
            v = 0.1 * torch.randn(shape, generator=g)
        else:
            v = (0.5 if ".t_cond." in name else 1.0) * torch.randn(shape, generator=g) / int(np.prod(shape[1:])) ** 0.5
        sd[name] = v
    return sd


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


def res_operands(case, seed=1700):
    """(ResBlock with seeded parameters, x (B, C, T, H, W), emb (B, 2C) or None), float32 on the CPU."""
    from autoregressive_diffusion_amd.vae import ResBlock
    B, T, H, W, C, g, with_emb = case
    rb = seed_module(ResBlock(C, (2 * g, 3, 3), g, t_cond=False), seed)
    gen = torch.Generator().manual_seed(seed + 1)
    return rb, _randn(gen, B, C, T, H, W), (0.5 * _randn(gen, B, 2 * C) if with_emb else None)


def lin_vae(kind, p, seed=1710):
    """The smallest VAE whose first encoder block (down) or first decoder block (up, out) is the stage, so that the packed
    operands are those of VAE._pack_encoder / VAE._pack themselves; seeded, float32 on the CPU."""
    from autoregressive_diffusion_amd.vae import VAE
    if kind == "down":
        Cin, tc, sc, C = p
        vae = VAE(channels=[Cin, C], n_res_blocks=1, time_compressions=[tc], spatial_compressions=[sc])
    elif kind == "up":
        C, tc, sc = p
        vae = VAE(channels=[1, C], n_res_blocks=1, time_compressions=[tc], spatial_compressions=[sc])
    elif kind == "out_last":
        C, Cout = p
        vae = VAE(channels=[Cout // 2, C], n_res_blocks=1, time_compressions=[1], spatial_compressions=[1])
    else:
        C, Cout = p
        vae = VAE(channels=[1, Cout, C], n_res_blocks=1, time_compressions=[1, 1], spatial_compressions=[1, 1])
    return seed_module(vae, seed)


def lin_input(kind, p, grid, seed=1711):
    """The stage's input, channels-first (B, C, T, H, W), float32 on the CPU."""
    B, T, H, W = grid
    gen = torch.Generator().manual_seed(seed)
    if kind == "down":
        Cin, tc, sc, _ = p
        return _randn(gen, B, Cin, T * tc, H * sc, W * sc)
    return _randn(gen, B, p[0], T, H, W)


def lin_operands(kind, name):
    """A 1x1 case by kind ("down", "up", "out") and name: (its VAE, the stage's conv module in it, x, tc, sc, the
    logvar_multiplier parameter for the last Out block or None), float32 on the CPU."""
    p, grid, flag = dict(down=DOWN_CASES, up=UP_CASES, out=OUT_CASES)[kind][name]
    last = kind == "out" and flag
    vae = lin_vae("out_last" if last else kind, p)
    blk = vae.encoder.encoder_blocks[0] if kind == "down" else vae.decoder.encoder_blocks[0]
    conv = blk.compression_block if kind == "down" else blk.decompression_block if kind == "up" else blk.final_conv
    tc, sc = (p[1], p[2]) if kind != "out" else (1, 1)
    return vae, conv, lin_input(kind, p, grid), tc, sc, (vae.decoder.logvar_multiplier if last else None)


# ---- the oracle: the restatement's formulas under autograd, in any dtype
def _backward(outs, leaves, dtype):
    sum((o * RT.cotangents(o.shape, phi, dtype)).sum() for o, phi in zip(outs.values(), RT.PHIS)).backward()
    return {k: o.detach() for k, o in outs.items()}, {"d" + k: v.grad for k, v in leaves.items()}


def _leaves(tensors, dtype):
    return {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in tensors.items() if v is not None}


def res_oracle(rb, x, emb, g, dtype, block=None):
    """out and dx, demb, dwa, dba, dwb, dbb of a ResBlock in `dtype`; block: the restatement's _res_block or a defective one."""
    L = _leaves(dict(x=x, emb=emb, wa=rb.conv3d0.conv3d.weight, ba=rb.conv3d0.conv3d.bias, wb=rb.conv3d1.weight,
                     bb=rb.conv3d1.bias), dtype)
    sd = {"conv3d0.conv3d.weight": L["wa"], "conv3d0.conv3d.bias": L["ba"], "conv3d1.weight": L["wb"], "conv3d1.bias": L["bb"]}
    out = (block or RT._res_block)(sd, "", L["x"], g, None, L.get("emb"))
    return _backward(dict(out=out), L, dtype)


def lin_oracle(kind, x, weight, bias, tc, sc, dtype, lvm=None, fn=None):
    """y and dx, dw, db of a 1x1 stage in `dtype` (out_last: mean, logvar and dlvm too); fn: RT.down / RT.up / RT.out or a
    defective one."""
    L = _leaves(dict(x=x, w=weight, b=bias, lvm=lvm), dtype)
    if kind == "down":
        outs = dict(y=(fn or RT.down)(L["x"], L["w"], L["b"], tc, sc))
    elif kind == "up":
        outs = dict(y=(fn or RT.up)(L["x"], L["w"], L["b"], tc, sc))
    else:
        y = (fn or RT.out)(L["x"], L["w"], L["b"])
        outs = dict(y=y)
        if lvm is not None:
            mean, logvar = y.split(y.shape[1] // 2, dim=1)
            outs = dict(mean=mean, logvar=logvar * torch.exp(L["lvm"]))
    return _backward(outs, L, dtype)


# ---- metrics and bounds
def metrics(a, ref):
    """(rel L2, max |a - ref| / rms(ref)) against ref in float64."""
    a, ref = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    d = a - ref
    return (d.norm() / ref.norm()).item(), (d.abs().max() / ref.pow(2).mean().sqrt()).item()


def bounds(ref64, ref32):
    """Per kind (outputs, gradients) the bounds (rel L2, max / rms) = FACTOR x the worst figure of the float32 oracle against the
    float64 one over the tensors of that kind, the rel L2 bound capped at OUT_TOL / GRAD_TOL; and the float32 figures."""
    fig32 = [{k: metrics(r32[k], r64[k]) for k in r64} for r64, r32 in zip(ref64, ref32)]
    bnd = []
    for figs, cap in zip(fig32, (OUT_TOL, GRAD_TOL)):
        bnd.append((min(FACTOR * max(f[0] for f in figs.values()), cap), FACTOR * max(f[1] for f in figs.values())))
    return bnd, fig32


def compare(what, got, ref64, ref32, in_order=None):
    """Every tensor of got = (outputs, gradients) against the float64 oracle under both metrics; prints each figure next to the
    float32 oracle's, then returns the failures (empty: the case passes).  in_order: {name: the float32 emulation of the
    kernel's own summation order} for the tensors of KERNEL_ORDER -- such a tensor is held to the same two bounds against the
    emulation, and the emulation to the ceiling GRAD_TOL against float64; its float64 figure is still printed."""
    bnd, fig32 = bounds(ref64, ref32)
    bad = []
    for g, r64, f32, (brel, bmax) in zip(got, ref64, fig32, bnd):
        assert set(g) == set(r64), (what, sorted(g), sorted(r64))
        for k in r64:
            assert float(r64[k].abs().max()) > 0, (what, k, "the oracle's tensor is identically zero")
            rel, mx = metrics(g[k], r64[k])
            line = (f"{what} {k:7s} rel {rel:.2e} (float32 {f32[k][0]:.2e}, bound {brel:.2e})   "
                    f"max/rms {mx:.2e} (float32 {f32[k][1]:.2e}, bound {bmax:.2e})")
            if in_order and k in in_order:
                anchor = metrics(in_order[k], r64[k])
                rel, mx = metrics(g[k], in_order[k])
                line += (f"   -> held to the float32 emulation of the kernel's order: rel {rel:.2e} max/rms {mx:.2e}; the emulation "
                         f"against float64: rel {anchor[0]:.2e} (ceiling {GRAD_TOL:.0e}) max/rms {anchor[1]:.2e}")
                if not anchor[0] <= GRAD_TOL:
                    bad.append(line)
            print(line)
            if not (rel <= brel and mx <= bmax):
                bad.append(line)
    return bad


# ---- a sum whose order decides: the bias gradient of conv B is, with this file's cotangent, sum over (t, h, w) of
# cos(0.7 i + phi), terms of size one that cancel to a sum of size one.  The float32 oracle adds them pairwise; the kernel
# (csrc/vae_train.hip vt_wgrad3_kernel) adds the 256 pixels of a tile one after the other, then the items of a slab, then the
# slabs.  At r06 (1728 terms per channel, 96 + 12 per frame) that order alone puts the kernel at 5.0e-06 from float64, ten
# times the float32 oracle's 4.9e-07 and twice the bound, on either slab policy (profiles/vae_stage_tests.txt).  The cotangent
# is the operand itself, so the order can be replayed exactly (the kernel's dbb equals the replay bit for bit): dbb of r06 is
# compared with that replay, every other tensor of every case, dbb included, with float64.
KERNEL_ORDER = {"r06": ("dbb",)}


def bias_grad_in_kernel_order(dout, nslab):
    """d bias of conv B as vt_wgrad3_kernel sums it, in float32 on the CPU: dout (B, C, T, H, W) -> (C,).  Work item
    (b, frame, 16x16 tile): its 256 pixels in row order from zero; slab s: the items s, s + nslab, ... in that order; then the
    slabs, slab 0 first."""
    B, C, T, H, W = dout.shape
    ty, tx = -(-H // 16), -(-W // 16)
    d = F.pad(dout.float(), (0, tx * 16 - W, 0, ty * 16 - H))
    d = d.reshape(B, C, T, ty, 16, tx, 16).permute(0, 2, 3, 5, 4, 6, 1).reshape(B * T * ty * tx, 256, C)
    s = torch.zeros(d.shape[0], C)
    for p in range(256):
        s = s + d[:, p]
    slab = torch.zeros(nslab, C)
    for i in range(0, s.shape[0], nslab):
        part = s[i:i + nslab]
        slab[:part.shape[0]] = slab[:part.shape[0]] + part
    out = torch.zeros(C)
    for i in range(nslab):
        out = out + slab[i]
    return out


# ---- the restatement with one defect at a time (defect None: the restatement itself, which the CPU tests assert)
RES_DEFECTS = ("prefix_attached", "prefix_zero", "halo_column", "interleave")
LIN_DEFECTS = ("hc_wc", "area_floor")


def _drop_halo_column(conv, seq):
    """conv over a padded operand as a tile kernel that never stages the last halo column of a 16-wide tile: the outputs of
    column 15 of a tile do not see the column to their right."""
    full = conv(seq)
    W = full.shape[-1]
    cols = [c for c in range(15, W - 1, 16)]
    if not cols:
        return full
    cut = seq.clone()
    cut[..., [c + 2 for c in cols]] = 0              # padded coordinates: image column c + 1 sits at c + 2
    mask = torch.zeros(W, dtype=torch.bool)
    mask[cols] = True
    return torch.where(mask, conv(cut), full)


def res_block_defect(defect):
    """RT._res_block with `defect` (one of RES_DEFECTS, or None)."""
    assert defect is None or defect in RES_DEFECTS

    def block(sd, q, x, g, t, emb=None):
        B, C, T, H, W = x.shape
        y = RT._rms(x)
        if emb is not None:
            y = y * (1 + emb[:, :C, None, None, None]) + emb[:, C:, None, None, None]
        yp = F.pad(F.silu(y), (1, 1, 1, 1))
        prefix = yp[:, :, :g].detach()
        if defect == "prefix_attached":
            prefix = yp[:, :, :g]
        if defect == "prefix_zero":
            prefix = torch.zeros_like(prefix)
        seq = torch.cat((prefix, yp), dim=2)
        conv_a = lambda s: F.conv3d(s, sd[q + "conv3d0.conv3d.weight"], sd[q + "conv3d0.conv3d.bias"], stride=(g, 1, 1))
        y = _drop_halo_column(conv_a, seq) if defect == "halo_column" else conv_a(seq)
        if defect == "interleave":
            y = y.reshape(B, C, g, T // g, H, W).reshape(B, C, T, H, W)                     # '(c g) t -> c (g t)'
        else:
            y = y.reshape(B, C, g, T // g, H, W).permute(0, 1, 3, 2, 4, 5).reshape(B, C, T, H, W)
        y = F.silu(RT._rms(y))
        conv_b = lambda s: F.conv3d(s, sd[q + "conv3d1.weight"], sd[q + "conv3d1.bias"])
        yp = F.pad(y, (1, 1, 1, 1))
        return x + (_drop_halo_column(conv_b, yp) if defect == "halo_column" else conv_b(yp))
    return block


def _area_defect(x, cout, defect):
    cin = x.shape[1]
    outs = []
    for o in range(cout):
        s0 = (o * cin) // cout
        s1 = ((o + 1) * cin) // cout if defect == "area_floor" else -((-(o + 1) * cin) // cout)
        outs.append(x[:, s0:s1].mean(dim=1))
    return torch.stack(outs, dim=1)


def lin_defect(kind, defect):
    """RT.down / RT.up / RT.out with `defect` (one of LIN_DEFECTS, or None)."""
    assert defect is None or defect in LIN_DEFECTS
    swap = defect == "hc_wc"

    def down(x, weight, bias, tc, sc):
        B, C, T, H, W = x.shape
        T, H, W = T // tc, H // sc, W // sc
        x = x.reshape(B, C, T, tc, H, sc, W, sc).permute(*((0, 3, 7, 5, 1, 2, 4, 6) if swap else (0, 3, 5, 7, 1, 2, 4, 6)))
        x = x.reshape(B, tc * sc * sc * C, T, H, W)
        return F.conv3d(x, weight, bias) + _area_defect(x, weight.shape[0], defect)

    def up(x, weight, bias, tc, sc):
        C = x.shape[1]
        x = F.conv3d(x, weight, bias)
        B, _, T, H, W = x.shape
        x = x.reshape(B, tc, sc, sc, C, T, H, W).permute(*((0, 4, 5, 1, 6, 3, 7, 2) if swap else (0, 4, 5, 1, 6, 2, 7, 3)))
        return x.reshape(B, C, T * tc, H * sc, W * sc)

    def out(x, weight, bias):
        return F.conv3d(x, weight, bias) + _area_defect(x, weight.shape[0], defect)
    return dict(down=down, up=up, out=out)[kind]
