"""The differentiable path of `vae.VAE.forward`: one autograd Function per stage of the VAE, each a few launches of csrc/vae_train.hip
(backward, and the ResBlock's training forward: the tile kernel of csrc/vae_conv3.h, which inference runs too) and of the
inference kernels (the forward of the 1x1 stages), so that the encoder's training forward is bit-identical to `VAE.encode`.
Activations travel between the stages channels-last [B][T][H][W][C] fp32.  What stays in torch is plumbing at parameter or latent
size: the t-embedding (MPFourier -> t_cond, under autograd), the mix of mean and noise, the permutations between the kernels'
weight layouts and the parameters' and the channels-first <-> channels-last copies at the two ends (include/oniris.h:
oniris_vae_train_*, oniris_vae_*_bwd).

Gradients are summed in a fixed order into a bounded number of partial slabs and then over the slabs; nothing uses atomics."""
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


def run(vae, x, t_b, noise):
    """The training forward of VAE.forward: x (B, 3, T, H, W) on the GPU, t_b (B,), noise (the shape of mean) or None (drawn after
    the encode, as in the reference) -> (r_mean, r_logvar, mean), attached to the autograd graph of the VAE's parameters."""
    from .edm2.utils import bmult
    dev = x.device
    epk, dpk = vae._pack_encoder(dev), vae._pack(dev)
    y = x.float().permute(0, 2, 3, 4, 1)
    for blk, bk in zip(vae.encoder.encoder_blocks, epk["blocks"]):
        y = Down.apply(y, blk.compression_block.weight, blk.compression_block.bias, bk)
        for rb, pk in zip(blk.res_blocks, bk["res"]):
            y = Res.apply(y, None, rb.conv3d0.conv3d.weight, rb.conv3d0.conv3d.bias, rb.conv3d1.weight, rb.conv3d1.bias, bk, pk)
    mean = y.permute(0, 4, 1, 2, 3).contiguous()
    if noise is None:
        noise = torch.randn_like(mean)
    z = bmult(mean, 1 - t_b) + bmult(noise, t_b)
    y = z.permute(0, 2, 3, 4, 1)
    nblk = len(dpk["blocks"])
    for i, (blk, bk) in enumerate(zip(vae.decoder.encoder_blocks, dpk["blocks"])):
        y = Up.apply(y, blk.decompression_block.weight, blk.decompression_block.bias, bk)
        for rb, pk in zip(blk.res_blocks, bk["res"]):
            emb = rb.t_cond(rb.fourier_cond(t_b))
            y = Res.apply(y, emb, rb.conv3d0.conv3d.weight, rb.conv3d0.conv3d.bias, rb.conv3d1.weight, rb.conv3d1.bias, bk, pk)
        if i < nblk - 1:
            y = Out.apply(y, blk.final_conv.weight, blk.final_conv.bias, None, bk, None)
        else:
            r_mean, r_logvar = Out.apply(y, blk.final_conv.weight, blk.final_conv.bias, vae.decoder.logvar_multiplier, bk, dpk["lvm"])
    return r_mean, r_logvar, mean
