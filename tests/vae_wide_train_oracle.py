"""Float64 references for the backward of the wide VAE stages (autoregressive_diffusion_amd/vae_train.py: Res, Down, Up, Out
on a wide packed block): Python restatements of the indexing of the kernels that run the data gradients on repacked weights, so that a
packing layout can be judged on the CPU, and the stages of tests/vae_train_cpu_restatement.py under autograd in float64 (the
reference) and float32 (whose distance from float64 sets the bounds).  Nothing here launches a kernel."""
import torch
import torch.nn.functional as F

import vae_train_cpu_restatement as RT
import vae_wide_oracle as O  # noqa: F401
import vae_wide_encoder_oracle as E

F64 = torch.float64


# ---- the kernels' indexing on packed operands (csrc/vae_wide_conv.h), channels-last float64

def conv_a_packed(S, w, bias, g, C):
    """vae_wide_kernel<NB, VW_CONV_A>: out[b, tau g + gl, y, x, c] = bias[gl][c] + sum_{kt < 2g, ky, kx, ci} w[kt][ky][kx][ci][gl][c]
    S[b, tau g + kt, y + ky - 1, x + kx - 1, ci]; S (B, g + T, H, W, C), w (2g, 3, 3, CinP, g, CP), bias (g, CP)."""
    B, TS, H, W, _ = S.shape
    T = TS - g
    Sp = F.pad(S.to(F64), (0, 0, 1, 1, 1, 1))
    w, out = w.to(F64), torch.zeros(B, T, H, W, C, dtype=F64)
    for tau in range(T // g):
        for kt in range(2 * g):
            for ky in range(3):
                for kx in range(3):
                    out[:, tau * g:(tau + 1) * g] += torch.einsum("bhwi,igc->bghwc", Sp[:, tau * g + kt, ky:ky + H, kx:kx + W, :C],
                                                                  w[kt, ky, kx, :C, :, :C])
    return out + bias.to(F64)[None, :, None, None, :C].repeat(1, T // g, 1, 1, 1)


def conv3_packed(x, w, C):
    """disc_conv_kernel at 9 taps without bias: out[b, t, y, x, c] = sum_{ky, kx, ci} w[ky][kx][ci][c] x[b, t, y + ky - 1, x + kx - 1, ci];
    w (3, 3, CinP, CP)."""
    H, W = x.shape[2:4]
    xp = F.pad(x.to(F64), (0, 0, 1, 1, 1, 1))
    return sum(torch.einsum("bthwi,ic->bthwc", xp[:, :, ky:ky + H, kx:kx + W, :C], w.to(F64)[ky, kx, :C, :C])
               for ky in range(3) for kx in range(3))


def up_packed(x, w, bias, Cin, Cout, tc, sc):
    """vae_wide_kernel<NB, VW_UP>: out[b, t tc + tq, y sc + hq, x sc + wq, c] = bias[sub][c] + sum_ci x[b, t, y, x, ci] w[ci][sub][c],
    sub = (tq sc + hq) sc + wq; w (CinP, nsub, CP), bias (nsub, CP)."""
    B, T, H, W, _ = x.shape
    y = torch.einsum("bthwi,isc->bthwsc", x.to(F64), w.to(F64)[:Cin, :, :Cout]) + bias.to(F64)[:, :Cout]
    y = y.reshape(B, T, H, W, tc, sc, sc, Cout).permute(0, 1, 4, 2, 5, 3, 6, 7)
    return y.reshape(B, T * tc, H * sc, W * sc, Cout)


def down_packed(x, w, bias, Cin, Cout, tc, sc):
    """vae_wide_down_kernel without the residual: out[b, t, y, x, o] = bias[o] + sum_{pos, c} x[b, t tc + tq, y sc + hq, x sc + wq, c]
    w[pos][c][o], pos = (tq sc + hq) sc + wq; w (npos, CinP, CP), bias (CP)."""
    r = E.rearrange_down(x.to(F64), tc, sc)
    r = r.reshape(*r.shape[:4], tc * sc * sc, Cin)
    return torch.einsum("bthwpc,pco->bthwo", r, w.to(F64)[:, :Cin, :Cout]) + bias.to(F64)[:Cout]


# ---- linear stages of the float64 oracles under autograd (the pack tests), channels-last

def lin_grads(stage, x, weight, bias, douts, **kw):
    """(outputs, dx, d weight, d bias) of sum_k sum(out_k dout_k) for stage(x, weight, bias, **kw) -> an output or a tuple."""
    x, weight, bias = [t.detach().double().clone().requires_grad_(True) for t in (x, weight, bias)]
    outs = stage(x, weight, bias, **kw)
    outs = outs if isinstance(outs, tuple) else (outs,)
    sum((o * d.double()).sum() for o, d in zip(outs, douts)).backward()
    return tuple(o.detach() for o in outs), x.grad, weight.grad, bias.grad


# ---- the training restatement's stages (tests/vae_train_cpu_restatement.py) under autograd in any dtype, channels-first on the
# CPU, with given cotangents: the reference (float64) and its float32 evaluation, whose distance sets the bounds

def _run(fn, tensors, cots, dtype):
    L = {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in tensors.items() if v is not None}
    outs = fn(L)
    sum((o * c.detach().cpu().to(dtype)).sum() for o, c in zip(outs.values(), cots)).backward()
    return {k: o.detach() for k, o in outs.items()}, {"d" + k: v.grad for k, v in L.items()}


def res_ref(x, emb, wa, ba, wb, bb, g, dout, dtype):
    """x, dout (B, C, T, H, W); -> ({out}, {dx, demb, dwa, dba, dwb, dbb})."""
    def fn(L):
        sd = {"conv3d0.conv3d.weight": L["wa"], "conv3d0.conv3d.bias": L["ba"], "conv3d1.weight": L["wb"], "conv3d1.bias": L["bb"]}
        return dict(out=RT._res_block(sd, "", L["x"], g, None, L.get("emb")))
    return _run(fn, dict(x=x, emb=emb, wa=wa, ba=ba, wb=wb, bb=bb), (dout,), dtype)


def lin_ref(kind, x, w, b, tc, sc, douts, dtype, lvm=None):
    """kind "down" / "up" / "out"; x and douts channels-first; with lvm the outputs are (mean, logvar exp(lvm)) and dlvm is
    returned too.  -> ({y} or {mean, logvar}, {dx, dw, db[, dlvm]})."""
    def fn(L):
        if kind == "down":
            return dict(y=RT.down(L["x"], L["w"], L["b"], tc, sc))
        if kind == "up":
            return dict(y=RT.up(L["x"], L["w"], L["b"], tc, sc))
        y = RT.out(L["x"], L["w"], L["b"])
        if lvm is None:
            return dict(y=y)
        mean, logvar = y.split(y.shape[1] // 2, dim=1)
        return dict(mean=mean, logvar=logvar * torch.exp(L["lvm"]))
    return _run(fn, dict(x=x, w=w, b=b, lvm=lvm), douts, dtype)
