"""The differentiable path of `vae.VAE.forward`: one autograd Function per stage of the VAE, each a few launches of csrc/vae_train.hip
(backward, and the ResBlock's training forward: the tile kernel of csrc/vae_conv3.h, which inference runs too) and of the
inference kernels (the forward of the 1x1 stages), so that the encoder's training forward is bit-identical to `VAE.encode`.
Activations travel between the stages channels-last [B][T][H][W][C] fp32.  What stays in torch is plumbing at parameter or latent
size: the t-embedding (MPFourier -> t_cond, under autograd), the mix of mean and noise, the permutations between the kernels'
weight layouts and the parameters' and the channels-first <-> channels-last copies at the two ends (include/oniris.h:
oniris_vae_train_*, oniris_vae_*_bwd).

Gradients are summed in a fixed order into a bounded number of partial slabs and then over the slabs; nothing uses atomics.

A block wider than vae.MAX_NARROW runs WideRes / WideUp / WideOut / WideDown instead (below): the forward of csrc/vae_wide.hip and
the backward of csrc/vae_wide_train.hip, for a model on which VAE.wide_training() was called."""
import torch

from . import _lib, vae as V
from .vae import _area_windows, _gpt, _nch, _p, _slab_sum, _stream

_SLAB_BYTES = 64 << 20          # the most memory one launch's partial slabs may take
_area_cache = {}


def _nslab(work, size):
    """Partial slabs of `size` floats for `work` work items: one per item up to 1024, fewer when the slabs are large."""
    return int(max(1, min(work, 1024, max(64, _SLAB_BYTES // (4 * size)))))


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


class Down(torch.autograd.Function):
    """oniris_vae_down: x, a channels-last view (B, T tc, H sc, W sc, Cin) with any strides -> (B, T, H, W, Cout)."""

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
        bk, dy = ctx.bk, dy.contiguous()
        vx, vy = (bk["Cin"], bk["tc"], bk["sc"]), (bk["C"], 1, 1)
        dw = db = dx = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = _lin_dw(x.contiguous(), vx, dy, vy, ctx.grid)
            dw = dw.reshape(weight.shape)
        if ctx.needs_input_grad[0]:
            N, K = bk["C"], bk["Cin"] * bk["tc"] * bk["sc"] ** 2
            dx = _lin_dx(dy, vy, weight.detach().float().reshape(N, K) + _area(K, N, dy.device), vx, ctx.grid)
        return dx, dw, db, None


class Up(torch.autograd.Function):
    """oniris_vae_up: x, a channels-last view (B, T, H, W, C) with any strides -> (B, T tc, H sc, W sc, C)."""

    @staticmethod
    def forward(ctx, x, weight, bias, bk):
        B, T, H, W, C = x.shape
        up = V.up(x, x.stride(), (B, T, H, W), bk, _stream())
        ctx.save_for_backward(x, weight)
        ctx.bk, ctx.grid = bk, (B, T, H, W)
        return up

    @staticmethod
    def backward(ctx, dup):
        x, weight = ctx.saved_tensors
        bk, dup = ctx.bk, dup.contiguous()
        C = bk["C"]
        vx, vy = (C, 1, 1), (C, bk["tc"], bk["sc"])
        dw = db = dx = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = _lin_dw(x.contiguous(), vx, dup, vy, ctx.grid)
            dw = dw.reshape(weight.shape)
        if ctx.needs_input_grad[0]:
            dx = _lin_dx(dup, vy, weight.detach().float().reshape(-1, C), vx, ctx.grid)
        return dx, dw, db, None


class Out(torch.autograd.Function):
    """oniris_vae_out: x (B, T, H, W, C) -> (B, T, H, W, Cout) or, with logvar_multiplier (the last block), (mean, logvar), each
    (B, Cout / 2, T, H, W)."""

    @staticmethod
    def forward(ctx, x, weight, bias, lvm, bk, lvm32):
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
        C, Cout = bk["C"], bk["Cout"]
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
        vx, vy = (C, 1, 1), (Cout, 1, 1)
        dw = db = dx = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = _lin_dw(x, vx, dy, vy, ctx.grid)
            dw = dw.reshape(weight.shape)
        if ctx.needs_input_grad[0]:
            dx = _lin_dx(dy, vy, weight.detach().float().reshape(Cout, C) + _area(C, Cout, dy.device), vx, ctx.grid)
        return dx, dw, db, dlvm, None, None


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


class Res(torch.autograd.Function):
    """A ResBlock (vae.py:56-93) in training mode without a cache: x (B, T, H, W, C), emb (B, 2C) or None -> x + conv B(u)."""

    @staticmethod
    def forward(ctx, x, emb, wa, ba, wb, bb, bk, pk):
        B, T, H, W, C = x.shape
        g, nch, gpt = bk["g"], bk["nch"], bk["gpt"]
        s = _stream()
        x = x.contiguous()
        emb = None if emb is None else emb.detach().float().contiguous()
        a = torch.empty_like(x)
        _lib.check(_lib.lib.oniris_vae_train_res_a(_p(x), _p(emb), _p(pk["wa"]), _p(pk["ba"]), B, T, H, W, C, g, nch, gpt, _p(a), s),
                   "vae_train_res_a")
        out = torch.empty_like(x)
        _lib.check(_lib.lib.oniris_vae_train_res_b(_p(a), _p(x), _p(pk["wb"]), _p(pk["bb"]), B, T, H, W, C, nch, _p(out), s),
                   "vae_train_res_b")
        ctx.save_for_backward(x, a, wa, wb, *(() if emb is None else (emb,)))
        ctx.bk = bk
        return out

    @staticmethod
    def backward(ctx, dout):
        x, a, wa, wb = ctx.saved_tensors[:4]
        emb = ctx.saved_tensors[4] if len(ctx.saved_tensors) > 4 else None
        bk, dout = ctx.bk, dout.contiguous()
        B, T, H, W, C = x.shape
        g, nch, gpt = bk["g"], bk["nch"], bk["gpt"]
        s = _stream()
        dev = x.device
        wda, wdb = _pack_dgrad(wa, wb, C, g)
        tiles = -(-H // 16) * -(-W // 16)
        da = torch.empty_like(x)
        _lib.check(_lib.lib.oniris_vae_res_b_bwd(_p(dout), _p(a), _p(wdb), B, T, H, W, C, nch, _p(da), s), "vae_res_b_bwd")
        dwa = dba = dwb = dbb = demb = None
        if ctx.needs_input_grad[4] or ctx.needs_input_grad[5]:
            n = 9 * C * C + C
            nslab = _nslab(B * T * tiles, n)
            slab = torch.zeros(nslab, n, dtype=torch.float32, device=dev)
            _lib.check(_lib.lib.oniris_vae_conv3_wgrad_bwd(_p(a), None, _p(dout), B, T, H, W, C, 1, 0, _p(slab), nslab, s),
                       "vae_conv3_wgrad_bwd")
            r = _slab_sum(slab, n)
            dwb = r[:9 * C * C].view(3, 3, C, C).permute(3, 2, 0, 1).reshape(wb.shape)            # ky, kx, ci, c -> c, ci, 1, ky, kx
            dbb = r[9 * C * C:].clone()
        want_emb = emb is not None and ctx.needs_input_grad[1]
        part = torch.empty(tiles * (T // gpt), B, 2 * C, dtype=torch.float32, device=dev) if want_emb else None
        dx = torch.empty_like(x)
        _lib.check(_lib.lib.oniris_vae_res_a_bwd(_p(da), _p(x), _p(emb), _p(dout), _p(wda), B, T, H, W, C, g, nch, gpt, _p(dx),
                                                 _p(part), s), "vae_res_a_bwd")
        if want_emb:
            demb = _slab_sum(part, B * 2 * C).view(B, 2 * C)
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            nw = 2 * g * g * 9 * C * C
            n = nw + g * C
            nslab = _nslab(B * (T // g) * tiles, n)
            slab = torch.zeros(nslab, n, dtype=torch.float32, device=dev)
            _lib.check(_lib.lib.oniris_vae_conv3_wgrad_bwd(_p(x), _p(emb), _p(da), B, T, H, W, C, g, 1, _p(slab), nslab, s),
                       "vae_conv3_wgrad_bwd")
            r = _slab_sum(slab, n)
            dwa = r[:nw].view(2 * g, g, 3, 3, C, C).permute(5, 1, 4, 0, 2, 3).reshape(wa.shape)   # kt, gl, ky, kx, ci, c -> (c gl), ci, kt, ky, kx
            dba = r[nw:].view(g, C).t().reshape(-1)
        return dx, demb, dwa, dba, dwb, dbb, None, None


# ---------------------------------------------------------------------------------------------------------------------------------
# Blocks wider than vae.MAX_NARROW (and an encoder `down` that compresses more than vae.MAX_DOWN_K channels): the backward on the
# fp32 MFMA kernels of csrc/vae_wide_train.hip (include/oniris.h: oniris_vae_wide_*_bwd).  The forward is the inference launch
# sequence of csrc/vae_wide.hip without a cache.  The data-gradient layouts are packed once per parameter version: they live in the
# packed block / ResBlock of VAE._pack / VAE._pack_encoder, which are rebuilt when a parameter changes.

def _cp(c):
    return -(-c // 32) * 32


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


def _cached(pk, key, make):
    v = pk.get(key)
    if v is None:
        v = pk[key] = make()
    return v


def _wide_lin_dw(x, vx, dy, vy, grid, nslab=None):
    """d weight and d bias of a 1x1 stage on the MFMA weight-gradient loop: x a channels-last tensor with any strides, dy
    contiguous; vx / vy = (C, tc, sc) as in _lin_dw -> (dw [px][py][Cx][Cy], db [py][Cy])."""
    B, T, H, W = grid
    npx, npy = vx[1] * vx[2] ** 2, vy[1] * vy[2] ** 2
    nw = npx * npy * vx[0] * vy[0]
    n = nw + npy * vy[0]
    nslab = _nslab(B * T * -(-H // 16) * -(-W // 16), n) if nslab is None else nslab
    slab = torch.empty(nslab, n, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib.oniris_vae_wide_lin_wgrad_bwd(_p(x), *x.stride(), *vx, _p(dy), *vy, B, T, H, W, _p(slab), nslab, _stream()),
               "vae_wide_lin_wgrad_bwd")
    r = _slab_sum(slab, n)
    return r[:nw].view(npx, npy, vx[0], vy[0]), r[nw:].view(npy, vy[0])


def _wide_down_dx(dy, pack, grid, Cy, Cx, tc, sc):
    B, T, H, W = grid
    dx = torch.empty(B, T * tc, H * sc, W * sc, Cx, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib.oniris_vae_wide_down_bwd(_p(dy), _p(pack[0]), _p(pack[1]), _p(dx), B, T, H, W, Cy, Cx, tc, sc, _stream()),
               "vae_wide_down_bwd")
    return dx


class WideDown(torch.autograd.Function):
    """Down where the block's `down` is oniris_vae_wide_down (bk["wide_down"])."""

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
        bk, dy = ctx.bk, dy.contiguous()
        Cin, C, tc, sc = bk["Cin"], bk["C"], bk["tc"], bk["sc"]
        dw = db = dx = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = _wide_lin_dw(x, (Cin, tc, sc), dy, (C, 1, 1), ctx.grid)
            dw = dw[:, 0].permute(2, 0, 1).reshape(weight.shape)                       # pos, ci, co -> co, (pos ci)
            db = db.reshape(-1)
        if ctx.needs_input_grad[0]:
            pack = _cached(bk, "wd_dgrad", lambda: _pack_down_dgrad(weight, Cin, C, tc, sc))
            dx = _wide_down_dx(dy, pack, ctx.grid, C, Cin, tc, sc)
        return dx, dw, db, None


class WideUp(torch.autograd.Function):
    """Up of a wide block: oniris_vae_wide_up."""

    @staticmethod
    def forward(ctx, x, weight, bias, bk):
        x = x.contiguous()
        up = V.wide_up(x, bk, _stream())
        ctx.save_for_backward(x, weight)
        ctx.bk = bk
        return up

    @staticmethod
    def backward(ctx, dup):
        x, weight = ctx.saved_tensors
        bk, dup = ctx.bk, dup.contiguous()
        B, T, H, W, C = x.shape
        tc, sc = bk["tc"], bk["sc"]
        dw = db = dx = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = _wide_lin_dw(x, (C, 1, 1), dup, (C, tc, sc), (B, T, H, W))
            dw = dw[0].permute(0, 2, 1).reshape(weight.shape)                          # sub, ci, co -> (sub co), ci
            db = db.reshape(-1)
        if ctx.needs_input_grad[0]:
            pack = _cached(bk, "wu_dgrad", lambda: _pack_up_dgrad(weight, C, tc, sc))
            dx = torch.empty_like(x)
            _lib.check(_lib.lib.oniris_vae_wide_up_bwd(_p(dup), _p(pack[0]), _p(pack[1]), _p(dx), B, T, H, W, C, tc, sc, _stream()),
                       "vae_wide_up_bwd")
        return dx, dw, db, None


class WideOut(torch.autograd.Function):
    """Out of a wide block: oniris_vae_wide_out."""

    @staticmethod
    def forward(ctx, x, weight, bias, lvm, bk, lvm32):
        x = x.contiguous()
        ctx.bk, ctx.last = bk, lvm is not None
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
        C, Cout = bk["C"], bk["Cout"]
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
        grid = tuple(x.shape[:4])
        dw = db = dx = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = _wide_lin_dw(x, (C, 1, 1), dy, (Cout, 1, 1), grid)
            dw = dw[0, 0].t().reshape(weight.shape)
            db = db.reshape(-1)
        if ctx.needs_input_grad[0]:
            pack = _cached(bk, "wo_dgrad", lambda: _pack_down_dgrad(weight, C, Cout, 1, 1))
            dx = _wide_down_dx(dy, pack, grid, Cout, C, 1, 1)
        return dx, dw, db, dlvm, None, None


def _wide_act_bwd(x, emb, dy, add, dx, part):
    B, T, H, W, C = x.shape
    _lib.check(_lib.lib.oniris_vae_wide_act_bwd(_p(x), _p(emb), _p(dy), _p(add), _p(dx), _p(part), B, T, H, W, C, dx.shape[1], _stream()),
               "vae_wide_act_bwd")


def _wide_conv3_dw(xin, dA, B, T, H, W, C, g, causal, nslab=None):
    """The summed slab of oniris_vae_wide_conv3_wgrad_bwd -> (the weights, flat; the biases, flat)."""
    nw = (2 * g * g if causal else 1) * 9 * C * C
    n = nw + g * C
    nslab = _nslab(B * (T // g) * -(-H // 16) * -(-W // 16), n) if nslab is None else nslab
    slab = torch.empty(nslab, n, dtype=torch.float32, device=xin.device)
    _lib.check(_lib.lib.oniris_vae_wide_conv3_wgrad_bwd(_p(xin), xin.shape[1], _p(dA), dA.shape[1], B, T, H, W, C, g, int(causal), _p(slab),
                                                        nslab, _stream()), "vae_wide_conv3_wgrad_bwd")
    r = _slab_sum(slab, n)
    return r[:nw], r[nw:]


class WideRes(torch.autograd.Function):
    """Res at a width above MAX_NARROW: the forward is act, conv A, act, conv B of csrc/vae_wide.hip (VAE._res_blocks without a
    cache); x and a are kept, S and u are formed again in backward.  nslab (tests): the slab count of the two weight gradients."""

    @staticmethod
    def forward(ctx, x, emb, wa, ba, wb, bb, bk, pk, nslab=None):
        g, s = bk["g"], _stream()
        x = x.contiguous()
        emb = None if emb is None else emb.detach().float().contiguous()
        seq, _ = V.wide_act(x, s, _p(emb), None, g)
        a = V.wide_conv_a(seq, pk, g, s)
        u, _ = V.wide_act(a, s, out=seq.view(-1)[:x.numel()].view(x.shape))
        out = V.wide_conv_b(u, x, pk, s)
        ctx.save_for_backward(x, a, wa, wb, *(() if emb is None else (emb,)))
        ctx.bk, ctx.pk, ctx.nslab = bk, pk, nslab
        return out

    @staticmethod
    def backward(ctx, dout):
        x, a, wa, wb = ctx.saved_tensors[:4]
        emb = ctx.saved_tensors[4] if len(ctx.saved_tensors) > 4 else None
        bk, pk, dout = ctx.bk, ctx.pk, dout.contiguous()
        B, T, H, W, C = x.shape
        g, s = bk["g"], _stream()
        wda, wdb, zb = _cached(pk, "dgrad", lambda: _pack_dgrad_wide(wa, wb, C, g))
        need = ctx.needs_input_grad
        want_emb = emb is not None and need[1]
        dwa = dba = dwb = dbb = demb = dx = None
        if need[4] or need[5]:
            u, _ = V.wide_act(a, s)
            r, dbb = _wide_conv3_dw(u, dout, B, T, H, W, C, 1, False, ctx.nslab)
            dwb = r.view(3, 3, C, C).permute(3, 2, 0, 1).reshape(wb.shape)            # ky, kx, ci, c -> c, ci, 1, ky, kx
            del u
        if not (need[0] or want_emb or need[2] or need[3]):
            return None, None, None, None, dwb, dbb, None, None, None
        du = torch.empty_like(x)
        _lib.check(_lib.lib.oniris_vae_wide_conv_b_bwd(_p(dout), _p(wdb), _p(du), B, T, H, W, C, s), "vae_wide_conv_b_bwd")
        D = torch.empty(B, T + g, H, W, C, dtype=torch.float32, device=x.device)      # [da ++ g zero frames]
        D[:, T:].zero_()
        _wide_act_bwd(a, None, du, None, D, None)
        del du
        if need[2] or need[3]:
            S, _ = V.wide_act(x, s, _p(emb), None, g)
            r, dba = _wide_conv3_dw(S, D, B, T, H, W, C, g, True, ctx.nslab)
            dwa = r.view(2 * g, g, 3, 3, C, C).permute(5, 1, 4, 0, 2, 3).reshape(wa.shape)   # kt, gl, ky, kx, ci, c -> (c gl), ci, kt, ky, kx
            dba = dba.view(g, C).t().reshape(-1)
            del S
        if need[0] or want_emb:
            dy = V.wide_conv_a(D, dict(wa=wda, ba=zb), g, s)
            part = torch.empty(-(-T * H * W // 256), B, 2 * C, dtype=torch.float32, device=x.device) if want_emb else None
            dx = torch.empty_like(x)
            _wide_act_bwd(x, emb, dy, dout, dx, part)
            if want_emb:
                demb = _slab_sum(part, B * 2 * C).view(B, 2 * C)
        return dx, demb, dwa, dba, dwb, dbb, None, None, None


class _EmbValues(torch.autograd.Function):
    """emb with the values `values` (the same quantity as another fp32 evaluation gives it); the gradient passes to emb."""

    @staticmethod
    def forward(ctx, emb, values):
        return values.clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


def _res(wide, y, emb, rb, bk, pk):
    """One ResBlock on the kernels of its width."""
    w = (rb.conv3d0.conv3d.weight, rb.conv3d0.conv3d.bias, rb.conv3d1.weight, rb.conv3d1.bias)
    return WideRes.apply(y, emb, *w, bk, pk, None) if wide else Res.apply(y, emb, *w, bk, pk)


def run(vae, x, t_b, noise):
    """The training forward of VAE.forward: x (B, 3, T, H, W) on the GPU, t_b (B,), noise (the shape of mean) or None (drawn after
    the encode, as in the reference) -> (r_mean, r_logvar, mean), attached to the autograd graph of the VAE's parameters."""
    from .edm2.utils import bmult
    dev = x.device
    epk, dpk = vae._pack_encoder(dev), vae._pack(dev)
    y = x.float().permute(0, 2, 3, 4, 1)
    for blk, bk in zip(vae.encoder.encoder_blocks, epk["blocks"]):
        y = (WideDown if bk.get("wide_down") else Down).apply(y, blk.compression_block.weight, blk.compression_block.bias, bk)
        for rb, pk in zip(blk.res_blocks, bk["res"]):
            y = _res(bk.get("wide"), y, None, rb, bk, pk)
    mean = y.permute(0, 4, 1, 2, 3).contiguous()
    if noise is None:
        noise = torch.randn_like(mean)
    z = bmult(mean, 1 - t_b) + bmult(noise, t_b)
    y = z.permute(0, 2, 3, 4, 1)
    nblk, B = len(dpk["blocks"]), x.shape[0]
    # a model with a wide block: the values of every FiLM scale | shift are those of the inference launch (oniris_vae_wide_temb), so
    # that the decoder's forward is bit for bit the eval-mode one; the gradient still flows through the torch expression
    embk = V.wide_temb(dpk, vae._wide, t_b.contiguous(), _stream()) if vae._wide else None
    for i, (blk, bk) in enumerate(zip(vae.decoder.encoder_blocks, dpk["blocks"])):
        wide = bk["wide"]
        y = (WideUp if wide else Up).apply(y, blk.decompression_block.weight, blk.decompression_block.bias, bk)
        for rb, pk in zip(blk.res_blocks, bk["res"]):
            emb = rb.t_cond(rb.fourier_cond(t_b))
            if embk is not None:
                emb = _EmbValues.apply(emb, embk[B * pk["emb_off"]:B * (pk["emb_off"] + 2 * bk["C"])].view(B, 2 * bk["C"]))
            y = _res(wide, y, emb, rb, bk, pk)
        out = WideOut if wide else Out
        if i < nblk - 1:
            y = out.apply(y, blk.final_conv.weight, blk.final_conv.bias, None, bk, None)
        else:
            r_mean, r_logvar = out.apply(y, blk.final_conv.weight, blk.final_conv.bias, vae.decoder.logvar_multiplier, bk, dpk["lvm"])
    return r_mean, r_logvar, mean
