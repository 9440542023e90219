"""The differentiable path of `vae.VAE.forward`: one autograd Function per stage of the VAE, each a few launches of csrc/vae_train.hip
(backward, and the ResBlock's training forward: the tile kernel of csrc/vae_conv3.h, which inference runs too) and of the
inference kernels (the forward of the 1x1 stages), so that the encoder's training forward is bit-identical to `VAE.encode`.
Activations travel between the stages channels-last [B][T][H][W][C] fp32.  What stays in torch is plumbing at parameter or latent
size: the t-embedding (MPFourier -> t_cond, under autograd), the mix of mean and noise, the permutations between the kernels'
weight layouts and the parameters' and the channels-first <-> channels-last copies at the two ends (include/oniris.h:
oniris_vae_train_*, oniris_vae_*_bwd).

Gradients are summed in a fixed order into a bounded number of partial slabs and then over the slabs; nothing uses atomics.

Down, Up, Out and Res each serve both kernel families and read the family from the packed block they are given, as the launchers
of vae.py do.  A block wider than vae.MAX_NARROW (bk["wide"]; an encoder `down` that takes the GEMM: bk["wide_down"]) runs the
forward of csrc/vae_wide.hip, the inference launch sequence without a cache, and the backward on the fp32 MFMA kernels of
csrc/vae_wide_train.hip (include/oniris.h: oniris_vae_wide_*_bwd), for a model on which VAE.wide_training() was called.  Its
data-gradient layouts are packed once per parameter version: they live in the packed block / ResBlock of VAE._pack /
VAE._pack_encoder, which are rebuilt when a parameter changes."""
from types import SimpleNamespace

import torch

from . import _lib, vae as V
from .vae import _area_windows, _cp, _gpt, _nch, _p, _slab_sum, _stream

_SLAB_BYTES = 64 << 20          # the most memory one launch's partial slabs may take
_area_cache = {}


def _nslab(work, size, width=0):
    """Partial slabs of `size` floats for `work` work items: one per item up to 1024, fewer when the slabs are large, and never
    fewer than 64 for a stage of up to 256 channels (`width`: the stage's widest channel count).  Above 256 channels the floor
    is dropped, as discriminator._nslab27 does: one launch's slabs stay within _SLAB_BYTES, or it is a single slab where even
    one exceeds that (conv A at 512 channels and g = 4: 302 MB a slab).  Nothing is lost: a slab's grid alone, (time tap, frame,
    32-channel block) pairs by 32-channel blocks, is 162 workgroups at 257 channels and g = 1 and 8192 at 512 and g = 4."""
    if width > V.MAX_WIDTH:
        return int(max(1, min(work, 1024, _SLAB_BYTES // (4 * size))))
    return int(max(1, min(work, 1024, max(64, _SLAB_BYTES // (4 * size)))))


def _wide_slab_sum(slab, n, width):
    """_slab_sum; above 256 channels a single slab is the result and no launch is issued."""
    return slab[0] if slab.shape[0] == 1 and width > V.MAX_WIDTH else _slab_sum(slab, n)


def _cached(pk, key, make):
    v = pk.get(key)
    if v is None:
        v = pk[key] = make()
    return v


# ---------------------------------------------------------------------------------------------------------------------------------
# the 1x1 stages

def _area(K, N, device):
    """The channel-area residual (F.interpolate mode='area' over the channel axis, vae.py:136-141) as a matrix [N][K]."""
    key = (K, N, str(device))
    m = _area_cache.get(key)
    if m is None:
        m = torch.zeros(N, K, dtype=torch.float32)
        for o, (s0, s1) in enumerate(_area_windows(K, N)):
            m[o, s0:s1] = 1.0 / (s1 - s0)
        m = _area_cache[key] = m.to(device)
    return m


def _lin_dw(x, vx, dy, vy, grid):
    """d weight [N][K] and d bias [N] of a 1x1 stage; vx / vy = (C, tc, sc) views of x / dy over the coarse grid (B, T, H, W)."""
    K, N = vx[0] * vx[1] * vx[2] ** 2, vy[0] * vy[1] * vy[2] ** 2
    rows = grid[0] * grid[1] * grid[2] * grid[3]
    rpc = max(8, min(128, 12288 // (K + 1 + N)))
    nslab = _nslab(-(-rows // rpc), N * (K + 1))
    slab = torch.zeros(nslab, N * (K + 1), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib.oniris_vae_lin_dw_bwd(_p(x), *vx, _p(dy), *vy, *grid, _p(slab), nslab, _stream()), "vae_lin_dw_bwd")
    dw = _slab_sum(slab, N * (K + 1)).view(N, K + 1)
    return dw[:, :K], dw[:, K]


def _lin_dx(dy, vy, wc, vx, grid):
    """d input of a 1x1 stage, in the layout of the view vx."""
    B, T, H, W = grid
    dx = torch.empty(B, T * vx[1], H * vx[2], W * vx[2], vx[0], dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib.oniris_vae_lin_dx_bwd(_p(dy), *vy, _p(wc.contiguous()), _p(dx), *vx, B, T, H, W, _stream()), "vae_lin_dx_bwd")
    return dx


def _pack_down_dgrad(weight, Cin, Cout, tc, sc):
    """The adjoint of `down` (tc = sc = 1: of `out`) for oniris_vae_wide_down_bwd: (W + the area matrix)^T as an `up` weight."""
    npos = tc * sc * sc
    K = Cin * npos
    wc = weight.detach().float().reshape(Cout, K) + _area(K, Cout, weight.device)
    f32 = dict(dtype=torch.float32, device=weight.device)
    return V._pack_lin_wide(wc.t(), torch.zeros(K, **f32), Cout, Cin, npos, f32)


def _pack_up_dgrad(weight, C, tc, sc):
    """The adjoint of `up` for oniris_vae_wide_up_bwd: W^T as a `down` weight."""
    f32 = dict(dtype=torch.float32, device=weight.device)
    return V._pack_down_wide(weight.detach().float().reshape(-1, C).t(), torch.zeros(C, **f32), C, C, tc * sc * sc, f32)


def _wide_lin_dw(x, vx, dy, vy, grid, nslab=None):
    """d weight and d bias of a 1x1 stage on the MFMA weight-gradient loop: x a channels-last tensor with any strides, dy
    contiguous; vx / vy = (C, tc, sc) as in _lin_dw -> (dw [px][py][Cx][Cy], db [py][Cy])."""
    B, T, H, W = grid
    npx, npy = vx[1] * vx[2] ** 2, vy[1] * vy[2] ** 2
    nw = npx * npy * vx[0] * vy[0]
    n = nw + npy * vy[0]
    width = max(vx[0], vy[0])
    nslab = _nslab(B * T * -(-H // 16) * -(-W // 16), n, width) if nslab is None else nslab
    slab = torch.empty(nslab, n, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib.oniris_vae_wide_lin_wgrad_bwd(_p(x), *x.stride(), *vx, _p(dy), *vy, B, T, H, W, _p(slab), nslab, _stream()),
               "vae_wide_lin_wgrad_bwd")
    r = _wide_slab_sum(slab, n, width)
    return r[:nw].view(npx, npy, vx[0], vy[0]), r[nw:].view(npy, vy[0])


def _wide_down_dx(dy, pack, grid, Cy, Cx, tc, sc):
    B, T, H, W = grid
    dx = torch.empty(B, T * tc, H * sc, W * sc, Cx, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib.oniris_vae_wide_down_bwd(_p(dy), _p(pack[0]), _p(pack[1]), _p(dx), B, T, H, W, Cy, Cx, tc, sc, _stream()),
               "vae_wide_down_bwd")
    return dx


def _lin_bwd(need, x, dy, weight, vx, vy, grid, bk, wide, area, key):
    """The backward of a 1x1 stage: vx / vy = (C, tc, sc) views of x / dy over the coarse grid, area: whether the stage adds the
    channel-area residual (`down` and `out` do, and only `up` has the compression on dy's side), need: its needs_input_grad ->
    (dx in the layout of vx, dw, db in the parameters' shapes).  wide: on the MFMA kernels, with x in any strides and the
    data-gradient pack kept in bk under `key`; otherwise x is made contiguous and the weight is composed per call."""
    K, N = vx[0] * vx[1] * vx[2] ** 2, vy[0] * vy[1] * vy[2] ** 2
    dx = dw = db = None
    if need[1] or need[2]:
        if wide:
            dw, db = _wide_lin_dw(x, vx, dy, vy, grid)
            dw, db = dw.permute(1, 3, 0, 2), db.reshape(-1)                            # px, py, cx, cy -> (py cy), (px cx)
        else:
            dw, db = _lin_dw(x.contiguous(), vx, dy, vy, grid)
        dw = dw.reshape(weight.shape)
    if need[0] and not wide:
        wc = weight.detach().float().reshape(N, K)
        dx = _lin_dx(dy, vy, wc + _area(K, N, dy.device) if area else wc, vx, grid)
    elif need[0] and area:
        pack = _cached(bk, key, lambda: _pack_down_dgrad(weight, vx[0], vy[0], vx[1], vx[2]))
        dx = _wide_down_dx(dy, pack, grid, vy[0], vx[0], vx[1], vx[2])
    elif need[0]:
        pack = _cached(bk, key, lambda: _pack_up_dgrad(weight, vx[0], vy[1], vy[2]))
        dx = torch.empty_like(x)
        _lib.check(_lib.lib.oniris_vae_wide_up_bwd(_p(dy), _p(pack[0]), _p(pack[1]), _p(dx), *grid, vx[0], vy[1], vy[2], _stream()),
                   "vae_wide_up_bwd")
    return dx, dw, db


class Down(torch.autograd.Function):
    """oniris_vae_down, or oniris_vae_wide_down where bk["wide_down"]: x, a channels-last view (B, T tc, H sc, W sc, Cin) with any
    strides -> (B, T, H, W, Cout)."""

    @staticmethod
    def forward(ctx, x, weight, bias, bk):
        B, T, H, W = x.shape[0], x.shape[1] // bk["tc"], x.shape[2] // bk["sc"], x.shape[3] // bk["sc"]
        y = V.down(x, x.stride(), (B, T, H, W), False, bk, _stream())
        ctx.save_for_backward(x, weight)
        ctx.bk, ctx.grid = bk, (B, T, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        bk = ctx.bk
        vx, vy = (bk["Cin"], bk["tc"], bk["sc"]), (bk["C"], 1, 1)
        return *_lin_bwd(ctx.needs_input_grad, x, dy.contiguous(), weight, vx, vy, ctx.grid, bk, bk.get("wide_down"), True,
                         "wd_dgrad"), None


class Up(torch.autograd.Function):
    """oniris_vae_up: x, a channels-last view (B, T, H, W, C) with any strides -> (B, T tc, H sc, W sc, C); oniris_vae_wide_up
    where bk["wide"], which reads a contiguous x."""

    @staticmethod
    def forward(ctx, x, weight, bias, bk):
        if bk.get("wide"):
            x = x.contiguous()
        ctx.bk, ctx.grid = bk, tuple(x.shape[:4])
        up = V.up(x, x.stride(), ctx.grid, bk, _stream())
        ctx.save_for_backward(x, weight)
        return up

    @staticmethod
    def backward(ctx, dup):
        x, weight = ctx.saved_tensors
        bk = ctx.bk
        vx, vy = (bk["C"], 1, 1), (bk["C"], bk["tc"], bk["sc"])
        return *_lin_bwd(ctx.needs_input_grad, x, dup.contiguous(), weight, vx, vy, ctx.grid, bk, bk.get("wide"), False,
                         "wu_dgrad"), None


class Out(torch.autograd.Function):
    """oniris_vae_out, or oniris_vae_wide_out where bk["wide"]: x (B, T, H, W, C) -> (B, T, H, W, Cout) or, with
    logvar_multiplier (the last block), (mean, logvar), each (B, Cout / 2, T, H, W)."""

    @staticmethod
    def forward(ctx, x, weight, bias, lvm, bk, lvm32):
        if bk.get("wide"):
            x = x.contiguous()
        ctx.bk, ctx.grid, ctx.last = bk, tuple(x.shape[:4]), lvm is not None
        if lvm is None:
            y = V.out(x, bk, _stream())
            ctx.save_for_backward(x, weight)
            return y
        mean, logvar = V.out(x, bk, _stream(), lvm32, "moments")
        ctx.save_for_backward(x, weight, lvm, logvar)
        return mean, logvar

    @staticmethod
    def backward(ctx, *douts):
        bk = ctx.bk
        dlvm = None
        if ctx.last:
            x, weight, lvm, logvar = ctx.saved_tensors
            dm, dl = douts
            if ctx.needs_input_grad[3]:
                dlvm = (dl * logvar).sum().to(lvm.dtype).reshape(lvm.shape)          # logvar = raw exp(lvm)
            dy = torch.cat((dm, dl * torch.exp(lvm.detach().float())), dim=1).permute(0, 2, 3, 4, 1).contiguous()
        else:
            x, weight = ctx.saved_tensors
            dy = douts[0].contiguous()
        vx, vy = (bk["C"], 1, 1), (bk["Cout"], 1, 1)
        dx, dw, db = _lin_bwd(ctx.needs_input_grad, x, dy, weight, vx, vy, ctx.grid, bk, bk.get("wide"), True, "wo_dgrad")
        return dx, dw, db, dlvm, None, None


# ---------------------------------------------------------------------------------------------------------------------------------
# the ResBlock: per width one launch sequence, as five functions with the same shape (and one that packs the data-gradient
# weights); Res holds what the widths share
#   fwd(x, emb, bk, pk) -> (a, out)                              a: conv A's output, kept for backward
#   dwb(a, dout) -> (conv B's weight gradient, flat; its bias gradient, flat)
#   pack(wa, wb, C, g, pk) -> the data-gradient layouts of the two conv weights, for da and dx
#   da(dout, a, packs, bk) -> da, in whatever form dwa and dx read it
#   dwa(x, emb, da, g) -> (conv A's weight gradient, flat; its bias gradient, flat)
#   dx(da, x, emb, dout, packs, bk, want_emb) -> (dx, the partial sums of d emb or None)

def _pack_dgrad(wa, wb, C, g):
    """The data-gradient layouts of the two conv weights (include/oniris.h: oniris_vae_res_a_bwd / oniris_vae_res_b_bwd)."""
    nch, gpt = _nch(C), _gpt(C, g)
    f32 = dict(dtype=torch.float32, device=wa.device)
    w = wa.detach().float().reshape(C, g, C, 2 * g, 3, 3).flip(4, 5).permute(3, 1, 4, 5, 0, 2)     # kt, gl, ky, kx, c, ci
    w = torch.cat((w[g:], w[:g]), dim=1)                                  # r, j: j < g -> (gl j, kt g + r); j >= g -> (gl j - g, kt r)
    w = w.reshape(g // gpt, gpt, 2 * g, 3, 3, C, C).permute(0, 2, 3, 4, 5, 6, 1)                   # gq, j, ky, kx, c, ci, rl
    wda = torch.zeros(g // gpt, 2 * g, 3, 3, C, nch, gpt, **f32)
    wda[..., :C, :] = w
    wdb = torch.zeros(3, 3, C, nch, **f32)
    wdb[..., :C] = wb.detach().float()[:, :, 0].flip(2, 3).permute(2, 3, 0, 1)                     # ky, kx, co, ci
    return wda.contiguous(), wdb.contiguous()


def _conv3_dw(xin, emb, dA, g, causal):
    """The summed slab of oniris_vae_conv3_wgrad_bwd -> (the weights, flat; the biases, flat)."""
    B, T, H, W, C = xin.shape
    nw = (2 * g * g if causal else 1) * 9 * C * C
    n = nw + g * C
    nslab = _nslab(B * (T // g) * -(-H // 16) * -(-W // 16), n)
    slab = torch.zeros(nslab, n, dtype=torch.float32, device=xin.device)
    _lib.check(_lib.lib.oniris_vae_conv3_wgrad_bwd(_p(xin), _p(emb), _p(dA), B, T, H, W, C, g, int(causal), _p(slab), nslab, _stream()),
               "vae_conv3_wgrad_bwd")
    r = _slab_sum(slab, n)
    return r[:nw], r[nw:]


def _res_fwd(x, emb, bk, pk):
    B, T, H, W, C = x.shape
    g, nch, gpt, s = bk["g"], bk["nch"], bk["gpt"], _stream()
    a = torch.empty_like(x)
    _lib.check(_lib.lib.oniris_vae_train_res_a(_p(x), _p(emb), _p(pk["wa"]), _p(pk["ba"]), B, T, H, W, C, g, nch, gpt, _p(a), s),
               "vae_train_res_a")
    out = torch.empty_like(x)
    _lib.check(_lib.lib.oniris_vae_train_res_b(_p(a), _p(x), _p(pk["wb"]), _p(pk["bb"]), B, T, H, W, C, nch, _p(out), s),
               "vae_train_res_b")
    return a, out


def _res_dwb(a, dout):
    w, b = _conv3_dw(a, None, dout, 1, False)
    return w, b.clone()


def _res_da(dout, a, packs, bk):
    B, T, H, W, C = a.shape
    da = torch.empty_like(a)
    _lib.check(_lib.lib.oniris_vae_res_b_bwd(_p(dout), _p(a), _p(packs[1]), B, T, H, W, C, bk["nch"], _p(da), _stream()), "vae_res_b_bwd")
    return da


def _res_dx(da, x, emb, dout, packs, bk, want_emb):
    B, T, H, W, C = x.shape
    g, nch, gpt = bk["g"], bk["nch"], bk["gpt"]
    tiles = -(-H // 16) * -(-W // 16)
    part = torch.empty(tiles * (T // gpt), B, 2 * C, dtype=torch.float32, device=x.device) if want_emb else None
    dx = torch.empty_like(x)
    _lib.check(_lib.lib.oniris_vae_res_a_bwd(_p(da), _p(x), _p(emb), _p(dout), _p(packs[0]), B, T, H, W, C, g, nch, gpt, _p(dx),
                                             _p(part), _stream()), "vae_res_a_bwd")
    return dx, part


_NARROW_RES = SimpleNamespace(fwd=_res_fwd, dwb=_res_dwb, pack=lambda wa, wb, C, g, pk: _pack_dgrad(wa, wb, C, g), da=_res_da,
                              dwa=lambda x, emb, da, g: _conv3_dw(x, emb, da, g, True), dx=_res_dx)


def _pack_dgrad_wide(wa, wb, C, g):
    """The data-gradient layouts of a wide ResBlock's conv weights: conv A's for oniris_vae_wide_conv_a on D = [da ++ g zero
    frames] (tap j < g: (gl, kt) = (j, g + r); j >= g: (j - g, r), r the output frame in its group), conv B's for
    oniris_vae_wide_conv_b_bwd; both flipped in space and transposed."""
    CP, CinP = _cp(C), C + (C & 1)
    f32 = dict(dtype=torch.float32, device=wa.device)
    w = wa.detach().float().reshape(C, g, C, 2 * g, 3, 3).flip(4, 5).permute(3, 1, 4, 5, 0, 2)     # kt, gl, ky, kx, c, ci
    w = torch.cat((w[g:], w[:g]), dim=1)                                                           # r, j, ky, kx, c, ci
    wda = torch.zeros(2 * g, 3, 3, CinP, g, CP, **f32)
    wda[:, :, :, :C, :, :C] = w.permute(1, 2, 3, 4, 0, 5)                                          # j, ky, kx, c, r, ci
    wdb = torch.zeros(3, 3, CinP, CP, **f32)
    wdb[:, :, :C, :C] = wb.detach().float()[:, :, 0].flip(2, 3).permute(2, 3, 0, 1)                # ky, kx, co, ci
    return wda.contiguous(), wdb.contiguous(), torch.zeros(g, CP, **f32)


def _wide_act_bwd(x, emb, dy, add, dx, part):
    B, T, H, W, C = x.shape
    _lib.check(_lib.lib.oniris_vae_wide_act_bwd(_p(x), _p(emb), _p(dy), _p(add), _p(dx), _p(part), B, T, H, W, C, dx.shape[1], _stream()),
               "vae_wide_act_bwd")


def _wide_conv3_dw(xin, dA, B, T, H, W, C, g, causal, nslab=None):
    """The summed slab of oniris_vae_wide_conv3_wgrad_bwd -> (the weights, flat; the biases, flat)."""
    nw = (2 * g * g if causal else 1) * 9 * C * C
    n = nw + g * C
    nslab = _nslab(B * (T // g) * -(-H // 16) * -(-W // 16), n, C) if nslab is None else nslab
    slab = torch.empty(nslab, n, dtype=torch.float32, device=xin.device)
    _lib.check(_lib.lib.oniris_vae_wide_conv3_wgrad_bwd(_p(xin), xin.shape[1], _p(dA), dA.shape[1], B, T, H, W, C, g, int(causal), _p(slab),
                                                        nslab, _stream()), "vae_wide_conv3_wgrad_bwd")
    r = _wide_slab_sum(slab, n, C)
    return r[:nw], r[nw:]


# the wide sequence keeps x and a only: u and S are formed again in backward, each inside the function that reads it, so that u is
# freed before du is allocated, du before S and S before the last stage

def _wide_res_fwd(x, emb, bk, pk):
    """act, conv A, act, conv B of csrc/vae_wide.hip (vae.res without a cache)."""
    g, s = bk["g"], _stream()
    seq, _ = V.wide_act(x, s, _p(emb), None, g)
    a = V.wide_conv_a(seq, pk, g, s)
    u, _ = V.wide_act(a, s, out=seq.view(-1)[:x.numel()].view(x.shape))
    return a, V.wide_conv_b(u, x, pk, s)


def _wide_res_dwb(a, dout):
    u, _ = V.wide_act(a, _stream())
    return _wide_conv3_dw(u, dout, *a.shape, 1, False)


def _wide_res_da(dout, a, packs, bk):
    B, T, H, W, C = a.shape
    du = torch.empty_like(a)
    _lib.check(_lib.lib.oniris_vae_wide_conv_b_bwd(_p(dout), _p(packs[1]), _p(du), B, T, H, W, C, _stream()), "vae_wide_conv_b_bwd")
    D = torch.empty(B, T + bk["g"], H, W, C, dtype=torch.float32, device=a.device)      # [da ++ g zero frames]
    D[:, T:].zero_()
    _wide_act_bwd(a, None, du, None, D, None)
    return D


def _wide_res_dwa(x, emb, D, g):
    S, _ = V.wide_act(x, _stream(), _p(emb), None, g)
    return _wide_conv3_dw(S, D, *x.shape, g, True)


def _wide_res_dx(D, x, emb, dout, packs, bk, want_emb):
    B, T, H, W, C = x.shape
    dy = V.wide_conv_a(D, dict(wa=packs[0], ba=packs[2]), bk["g"], _stream())
    part = torch.empty(-(-T * H * W // 256), B, 2 * C, dtype=torch.float32, device=x.device) if want_emb else None
    dx = torch.empty_like(x)
    _wide_act_bwd(x, emb, dy, dout, dx, part)
    return dx, part


_WIDE_RES = SimpleNamespace(fwd=_wide_res_fwd, dwb=_wide_res_dwb, da=_wide_res_da, dwa=_wide_res_dwa, dx=_wide_res_dx,
                            pack=lambda wa, wb, C, g, pk: _cached(pk, "dgrad", lambda: _pack_dgrad_wide(wa, wb, C, g)))


class Res(torch.autograd.Function):
    """A ResBlock (vae.py:56-93) in training mode without a cache: x (B, T, H, W, C), emb (B, 2C) or None -> x + conv B(u), on
    the launch sequence of the block's width (bk["wide"]).  Backward forms only what was asked for, conv B's weight gradient
    first: a block of which only conv B trains stops there."""

    @staticmethod
    def forward(ctx, x, emb, wa, ba, wb, bb, bk, pk):
        k = _WIDE_RES if bk.get("wide") else _NARROW_RES
        x = x.contiguous()
        emb = None if emb is None else emb.detach().float().contiguous()
        a, out = k.fwd(x, emb, bk, pk)
        ctx.save_for_backward(x, a, wa, wb, *(() if emb is None else (emb,)))
        ctx.bk, ctx.pk, ctx.k = bk, pk, k
        return out

    @staticmethod
    def backward(ctx, dout):
        x, a, wa, wb = ctx.saved_tensors[:4]
        emb = ctx.saved_tensors[4] if len(ctx.saved_tensors) > 4 else None
        bk, k, need, dout = ctx.bk, ctx.k, ctx.needs_input_grad, dout.contiguous()
        B, C, g = x.shape[0], x.shape[4], bk["g"]
        want_emb = emb is not None and need[1]
        dx = demb = dwa = dba = dwb = dbb = None
        if need[4] or need[5]:
            r, dbb = k.dwb(a, dout)
            dwb = r.view(3, 3, C, C).permute(3, 2, 0, 1).reshape(wb.shape)            # ky, kx, ci, c -> c, ci, 1, ky, kx
        if not (need[0] or want_emb or need[2] or need[3]):
            return None, None, None, None, dwb, dbb, None, None
        packs = k.pack(wa, wb, C, g, ctx.pk)
        da = k.da(dout, a, packs, bk)
        if need[2] or need[3]:
            r, dba = k.dwa(x, emb, da, g)
            dwa = r.view(2 * g, g, 3, 3, C, C).permute(5, 1, 4, 0, 2, 3).reshape(wa.shape)   # kt, gl, ky, kx, ci, c -> (c gl), ci, kt, ky, kx
            dba = dba.view(g, C).t().reshape(-1)
        if need[0] or want_emb:
            dx, part = k.dx(da, x, emb, dout, packs, bk, want_emb)
            if want_emb:
                demb = _slab_sum(part, B * 2 * C).view(B, 2 * C)
        return dx, demb, dwa, dba, dwb, dbb, None, None


class _EmbValues(torch.autograd.Function):
    """emb with the values `values` (the same quantity as another fp32 evaluation gives it); the gradient passes to emb."""

    @staticmethod
    def forward(ctx, emb, values):
        return values.clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


def _convs(rb):
    return rb.conv3d0.conv3d.weight, rb.conv3d0.conv3d.bias, rb.conv3d1.weight, rb.conv3d1.bias


def run(vae, x, t_b, noise):
    """The training forward of VAE.forward: x (B, 3, T, H, W) on the GPU, t_b (B,), noise (the shape of mean) or None (drawn after
    the encode, as in the reference) -> (r_mean, r_logvar, mean), attached to the autograd graph of the VAE's parameters."""
    from .edm2.utils import bmult
    dev = x.device
    epk, dpk = vae._pack_encoder(dev, bf16=False), vae._pack(dev, bf16=False)    # VAE.bf16_inference() is for inference only
    y = x.float().permute(0, 2, 3, 4, 1)
    for blk, bk in zip(vae.encoder.encoder_blocks, epk["blocks"]):
        y = Down.apply(y, blk.compression_block.weight, blk.compression_block.bias, bk)
        for rb, pk in zip(blk.res_blocks, bk["res"]):
            y = Res.apply(y, None, *_convs(rb), bk, pk)
    mean = y.permute(0, 4, 1, 2, 3).contiguous()
    if noise is None:
        noise = torch.randn_like(mean)
    z = bmult(mean, 1 - t_b) + bmult(noise, t_b)
    y = z.permute(0, 2, 3, 4, 1)
    nblk, B = len(dpk["blocks"]), x.shape[0]
    # a model with a wide block: the values of every FiLM scale | shift are those of the inference launch (oniris_vae_wide_temb), so
    # that the decoder's forward is bit for bit the eval-mode one; the gradient still flows through the torch expression
    embk = V.temb(dpk, vae._wide, t_b.contiguous(), _stream()) if vae._wide else None
    for i, (blk, bk) in enumerate(zip(vae.decoder.encoder_blocks, dpk["blocks"])):
        y = Up.apply(y, blk.decompression_block.weight, blk.decompression_block.bias, bk)
        for rb, pk in zip(blk.res_blocks, bk["res"]):
            emb = rb.t_cond(rb.fourier_cond(t_b))
            if embk is not None:
                emb = _EmbValues.apply(emb, embk[B * pk["emb_off"]:B * (pk["emb_off"] + 2 * bk["C"])].view(B, 2 * bk["C"]))
            y = Res.apply(y, emb, *_convs(rb), bk, pk)
        if i < nblk - 1:
            y = Out.apply(y, blk.final_conv.weight, blk.final_conv.bias, None, bk, None)
        else:
            r_mean, r_logvar = Out.apply(y, blk.final_conv.weight, blk.final_conv.bias, vae.decoder.logvar_multiplier, bk, dpk["lvm"])
    return r_mean, r_logvar, mean
