"""VAE on HIP kernels: RGB frames -> latents, generated latents -> RGB frames, and the training forward / backward, on the GPU
(reference: edm2/vae/vae.py).

`VAE` has the reference's constructor, `kwargs` and state_dict keys (encoder and decoder), so a checkpoint of the reference's
VAE loads here unchanged and round-trips.  Encoder and decoder run for inference, in fp32 like the reference: `encode`,
`encode_long_sequence`, `frames_to_latents` and the streaming form `encode_frames`; `decode`, `latents_to_frames` and the
streaming form `decode_frames`.  Both are causal in time -- every group-causal conv keeps the last g activated frames of its
input as a cache (vae.py:18-53) -- so encoding or decoding a sequence chunk by chunk through the cache gives exactly what the
whole sequence gives (bit-identical here: csrc/vae*.hip and csrc/vae_conv3.h sum every output in a fixed order).
Activations are channels-last fp32 [B][T][H][W][C].  Decoder: per block one `up` launch, two per ResBlock, one `out` launch,
plus one t-embedding launch per decode.  Encoder: per block one `down` launch (uint8 frames are normalised on load) and two per
ResBlock (the decoder's kernels with a zero FiLM buffer), plus one `latents` launch per encode (include/oniris.h: oniris_vae_*).
Blocks wider than MAX_NARROW = 64 channels (up to MAX_WIDTH = 256; up to 512 in `VAE512`) run on the fp32 MFMA tile kernels of csrc/vae_wide.hip, on
both sides: the `up`, `out` and `down` stages as GEMMs and four launches per ResBlock (activation, conv A, activation, conv B; the
encoder passes a null FiLM pointer), with the same cache entries.  An encoder `down` also takes the GEMM when it compresses more
than 512 channels, whatever its output width.  A model that has such a block runs for inference only by default: the training
path of `forward` raises NotImplementedError until `VAE.wide_training()` switches it on for that model (include/oniris.h:
oniris_vae_wide_*, oniris_vae_wide_*_bwd).  `VAE512` is the same model for block widths up to 512 -- the full-size Counter-Strike VAE,
channels=[3, 32, 128, 512, 8] -- with the training path on as constructed; a model of up to 256 channels runs the same launches
under either class.  Above 256 channels conv A takes 128 output channels per workgroup where the padded width is a multiple of 128
(11.6 % faster at 512 channels than the 64-channel tile, same bits: profiles/vae_512.txt) and a weight-gradient launch keeps its partial slabs within 64 MiB, down to a
single slab that is the result (vae_train._nslab).

`VAE.bf16_inference()` switches the wide blocks of one model to bf16 MFMA operands for inference (csrc/vae_wide_bf16.hip,
include/oniris.h: oniris_vae_wide_*_bf16): the weights are rounded to bf16 (nearest even) when packed and the activated input of
conv A, conv B, `up`, `down` and `out` when a kernel stages it, each exactly once (every MFMA launch of the VAE: the GEMM `down` of a
narrow block that compresses more than MAX_DOWN_K channels among them); accumulation, biases, residuals (read from the unrounded
tensor), activations, caches and every tensor in HBM stay fp32, the register-tile kernels of the narrow blocks are untouched, and
the training path ignores the switch.  Off as constructed: the fp32 path keeps its bits and is the verification path (what `Precond(use_fp16=False)`
is for the UNet, with the default the other way round).

`forward` (encode, mix with noise, decode: what the reference's VAE training loops call) trains: in training mode with grad
enabled its outputs carry a grad_fn and `.backward()` fills `.grad` of every trainable parameter through the kernels of
csrc/vae_train.hip (vae_train.py).  Nothing here has a CPU path: use the reference's `edm2.vae` for that.
"""
import ctypes
import inspect

import numpy as np
import torch
from torch import nn

from . import _lib
from .edm2.utils import BetterModule, MPFourier, bmult

MAX_WIDTH = 256        # the widest block (the MFMA tile kernels of csrc/vae_wide.hip take any width; this is the one bound)
MAX_NARROW = 64        # up to here a block runs on the register-tile kernels of csrc/vae.hip / csrc/vae_conv3.h
MAX_DOWN_K = 512       # up to here a narrow encoder block's `down` runs on vae_down_kernel (csrc/vae_encoder.hip)
_REF = "the reference's edm2.vae (this package runs the VAE on HIP kernels only)"


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else t.data_ptr()


def _slab_sum(slab, n):
    """oniris_vae_slab_sum_bwd: the partial slabs slab[i] of n floats each -> their sum (n,), added in the order of i."""
    out = torch.empty(n, dtype=torch.float32, device=slab.device)
    _lib.check(_lib.lib.oniris_vae_slab_sum_bwd(_p(slab), slab.shape[0], n, _p(out), _stream()), "vae_slab_sum_bwd")
    return out


def _has_tensor(cache):
    """Whether a (nested) cache dict holds anything but None leaves."""
    if isinstance(cache, dict):
        return any(_has_tensor(v) for v in cache.values())
    return cache is not None


def _nch(c):
    """Channel capacity of the res-conv kernel instantiation that serves c channels: 8, 16, 32 or 64."""
    return next(n for n in (8, 16, 32, 64) if c <= n)


def _gpt(c, g):
    """Output frames per thread of res A: the largest power of two that divides g with nch * gpt <= 32 (csrc/vae_conv3.h)."""
    gpt = 1
    while gpt * 2 <= 4 and g % (gpt * 2) == 0 and _nch(c) * gpt * 2 <= 32:
        gpt *= 2
    return gpt


def _area_windows(K, N):
    """The windows (s0, s1) = [floor(o K / N), ceil((o + 1) K / N)) of F.interpolate mode='area' from K to N channels
    (interpolate_channels, vae.py:136-141), one per output channel o."""
    return [((o * K) // N, -((-(o + 1) * K) // N)) for o in range(N)]


def _cp(c):
    """c channels rounded up to a multiple of 32: the padded output width CP of csrc/vae_wide_conv.h."""
    return -(-c // 32) * 32


def _pack_res(rb, C, g, f32):
    """The two convolutions of a ResBlock in the layouts of vae_conv3_kernel (csrc/vae_conv3.h)."""
    nch, gpt = _nch(C), _gpt(C, g)
    w = rb.conv3d0.conv3d.weight.detach().to(**f32)                   # (C g, C, 2g, 3, 3), co = c g + gq gpt + gl
    w = w.reshape(C, g // gpt, gpt, C, 2 * g, 3, 3).permute(1, 4, 5, 6, 3, 0, 2)   # gq, kt, ky, kx, ci, c, gl
    wa = torch.zeros(g // gpt, 2 * g, 3, 3, C, nch, gpt, **f32)
    wa[:, :, :, :, :, :C] = w
    ba = torch.zeros(g // gpt, nch, gpt, **f32)
    ba[:, :C] = rb.conv3d0.conv3d.bias.detach().to(**f32).reshape(C, g // gpt, gpt).permute(1, 0, 2)
    wb = torch.zeros(3, 3, C, nch, **f32)
    wb[..., :C] = rb.conv3d1.weight.detach().to(**f32)[:, :, 0].permute(2, 3, 1, 0)   # ky, kx, ci, co
    bb = torch.zeros(nch, **f32)
    bb[:C] = rb.conv3d1.bias.detach().to(**f32)
    return dict(wa=wa.contiguous(), ba=ba.contiguous(), wb=wb.contiguous(), bb=bb)


def _cinp(c, bf16):
    """c input channels padded as the packed weights hold them: to even for the fp32 kernels (csrc/vae_wide_conv.h), to a multiple
    of 16, the K step of the MFMA, for the bf16 ones (csrc/vae_wide_bf16.h)."""
    return -(-c // 16) * 16 if bf16 else c + (c & 1)


def _wdtype(f32, bf16):
    """The tensor options of a wide block's packed weights: f32, or the same device in bf16.  A copy into such a tensor rounds to
    nearest even, as `weight.to(torch.bfloat16)` does -- the one rounding of the weights (csrc/vae_wide_bf16.h)."""
    return dict(f32, dtype=torch.bfloat16) if bf16 else f32


def _pack_res_wide(rb, C, g, f32, bf16=False):
    """The two convolutions of a ResBlock wider than MAX_NARROW in the layouts of csrc/vae_wide_conv.h: output channels
    [sub][CP] (CP = C rounded up to a multiple of 32), input channels rounded up to even, zero where padded.  bf16: the weights
    as bf16 in the same layouts with the input channels rounded up to a multiple of 16 (csrc/vae_wide_bf16.h), the biases fp32,
    and bf16=True in the dict, which is what makes wide_conv_a / wide_conv_b pick the bf16 entry points."""
    CP, CinP, wt = _cp(C), _cinp(C, bf16), _wdtype(f32, bf16)
    w = rb.conv3d0.conv3d.weight.detach().to(**f32)                   # (C g, C, 2g, 3, 3), co = c g + gl
    wa = torch.zeros(2 * g, 3, 3, CinP, g, CP, **wt)
    wa[:, :, :, :C, :, :C] = w.reshape(C, g, C, 2 * g, 3, 3).permute(3, 4, 5, 2, 1, 0)   # kt, ky, kx, ci, gl, c
    ba = torch.zeros(g, CP, **f32)
    ba[:, :C] = rb.conv3d0.conv3d.bias.detach().to(**f32).reshape(C, g).t()
    wb = torch.zeros(3, 3, CinP, CP, **wt)
    wb[:, :, :C, :C] = rb.conv3d1.weight.detach().to(**f32)[:, :, 0].permute(2, 3, 1, 0)   # ky, kx, ci, co
    bb = torch.zeros(CP, **f32)
    bb[:C] = rb.conv3d1.bias.detach().to(**f32)
    pk = dict(wa=wa.contiguous(), ba=ba.contiguous(), wb=wb.contiguous(), bb=bb)
    if bf16:
        pk["bf16"] = True
    return pk


def _pack_lin_wide(weight, bias, Cin, Cout, nsub, f32, bf16=False):
    """A 1x1 conv Cin -> nsub Cout (conv channel sub Cout + c) as w [CinP][nsub CP], bias [nsub][CP] (csrc/vae_wide_conv.h);
    bf16: w as bf16 with CinP a multiple of 16 (csrc/vae_wide_bf16.h)."""
    CP, CinP = _cp(Cout), _cinp(Cin, bf16)
    w = torch.zeros(CinP, nsub, CP, **_wdtype(f32, bf16))
    w[:Cin, :, :Cout] = weight.detach().to(**f32).reshape(nsub, Cout, Cin).permute(2, 0, 1)
    b = torch.zeros(nsub, CP, **f32)
    b[:, :Cout] = bias.detach().to(**f32).reshape(nsub, Cout)
    return w.contiguous(), b.contiguous()


def _pack_down_wide(weight, bias, Cin, Cout, npos, f32, bf16=False):
    """The compression 1x1 conv npos Cin -> Cout (rearranged channel k = pos Cin + c) as w [npos][CinP][CP], bias [CP]
    (vae_wide_down_kernel of csrc/vae_wide_conv.h); bf16: w as bf16 with CinP a multiple of 16 (csrc/vae_wide_bf16.h)."""
    CP, CinP = _cp(Cout), _cinp(Cin, bf16)
    w = torch.zeros(npos, CinP, CP, **_wdtype(f32, bf16))
    w[:, :Cin, :Cout] = weight.detach().to(**f32).reshape(Cout, npos, Cin).permute(1, 2, 0)
    b = torch.zeros(CP, **f32)
    b[:Cout] = bias.detach().to(**f32)
    return w.contiguous(), b


# ---------------------------------------------------------------------------------------------------------------------------------
# launches: thin wrappers on channels-last fp32 tensors (B, T, H, W, C) of the GPU, one per stage (temb, up, res, out, down: each
# picks the narrow or the wide entry point from the packed block it is given, and the wide one's bf16 form where the packed block
# or ResBlock says bf16=True) and one per entry point of a ResBlock.  bk: a packed
# block (VAE._pack, VAE._pack_encoder), rb: one of its packed ResBlocks, pk: the decoder's pack, dims: the coarse grid (B, T, H, W),
# strides: element strides (b, t, h, w, c) of an operand in any layout, s: the stream.  Each allocates what it writes and returns it.

def _new(x, *shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device=x.device)


def temb(pk, width, t, s):
    """oniris_vae_temb: t (B,) -> the FiLM scale | shift of every ResBlock, [ResBlock][B][2C] flat; oniris_vae_wide_temb for a
    model whose widest block has `width` > MAX_NARROW channels (0: none has; the narrow kernel holds the Fourier features of 64)."""
    emb = _new(t, t.shape[0] * pk["emb_per_row"])
    head = (_p(pk["tparams"]), _p(pk["table"]), pk["n_rb"])
    if width:
        _lib.check(_lib.lib.oniris_vae_wide_temb(*head, 2 * width, _p(t), t.shape[0], _p(emb), s), "vae_wide_temb")
    else:
        _lib.check(_lib.lib.oniris_vae_temb(*head, _p(t), t.shape[0], _p(emb), s), "vae_temb")
    return emb


def _wide_entry(stage, pk):
    """(entry point, its name for error messages) of a wide stage: oniris_vae_wide_<stage>, or oniris_vae_wide_<stage>_bf16 where
    the packed block or ResBlock pk holds bf16 weights."""
    what = f"vae_wide_{stage}_bf16" if pk.get("bf16") else f"vae_wide_{stage}"
    return getattr(_lib.lib, "oniris_" + what), what


def up(x, strides, dims, bk, s, scale=None, shift=None):
    """oniris_vae_up: x over `dims` by `strides` (times scale plus shift per channel) -> (B, T tc, H sc, W sc, C); or
    oniris_vae_wide_up where bk["wide"]: x is then contiguous (`strides` is not read) and scale / shift are not taken."""
    B, T, H, W = dims
    C, tc, sc = bk["C"], bk["tc"], bk["sc"]
    y = _new(x, B, T * tc, H * sc, W * sc, C)
    if bk["wide"]:
        assert scale is None and shift is None and x.is_contiguous()
        entry, what = _wide_entry("up", bk)
        _lib.check(entry(_p(x), _p(bk["wu"]), _p(bk["bu"]), _p(y), B, T, H, W, C, tc, sc, s), what)
    else:
        _lib.check(_lib.lib.oniris_vae_up(_p(x), *strides, B, T, H, W, C, _p(scale), _p(shift), _p(bk["wu"]), _p(bk["bu"]), tc, sc,
                                          _p(y), s), "vae_up")
    return y


def res_a(x, cin, emb, rb, bk, s):
    """oniris_vae_res_a: x, the cache entry cin or None, the address emb of the FiLM scale | shift -> (u, the new cache entry)."""
    B, T, H, W, C = x.shape
    cout, u = _new(x, B, bk["g"], H, W, C), torch.empty_like(x)
    _lib.check(_lib.lib.oniris_vae_res_a(_p(x), _p(cin), _p(cout), emb, _p(rb["wa"]), _p(rb["ba"]), B, T, H, W, C, bk["g"], bk["nch"],
                                         bk["gpt"], _p(u), s), "vae_res_a")
    return u, cout


def res_b(u, x, rb, bk, s):
    """oniris_vae_res_b: -> x + conv B(u)."""
    B, T, H, W, C = x.shape
    y = torch.empty_like(x)
    _lib.check(_lib.lib.oniris_vae_res_b(_p(u), _p(x), _p(rb["wb"]), _p(rb["bb"]), B, T, H, W, C, bk["nch"], _p(y), s), "vae_res_b")
    return y


def wide_act(x, s, emb=None, cin=None, g=0, out=None):
    """oniris_vae_wide_act: the activation of x (with FiLM where emb is an address), behind the g cached frames cin where g > 0
    -> (the sequence (B, g + T, H, W, C), written to `out` where given, the new cache entry or None)."""
    B, T, H, W, C = x.shape
    cout = _new(x, B, g, H, W, C) if g else None
    out = _new(x, B, g + T, H, W, C) if out is None else out
    _lib.check(_lib.lib.oniris_vae_wide_act(_p(x), emb, _p(cin), _p(cout), _p(out), B, T, H, W, C, g, s), "vae_wide_act")
    return out, cout


def wide_conv_a(seq, rb, g, s):
    """oniris_vae_wide_conv_a (oniris_vae_wide_conv_a_bf16 where rb holds bf16 weights): the sequence (B, g + T, H, W, C) -> u
    (B, T, H, W, C)."""
    B, T, H, W, C = seq.shape[0], seq.shape[1] - g, *seq.shape[2:]
    u = _new(seq, B, T, H, W, C)
    entry, what = _wide_entry("conv_a", rb)
    _lib.check(entry(_p(seq), _p(rb["wa"]), _p(rb["ba"]), _p(u), B, T, H, W, C, g, s), what)
    return u


def wide_conv_b(a, x, rb, s):
    """oniris_vae_wide_conv_b (or its _bf16 form): -> x + conv B(a)."""
    B, T, H, W, C = x.shape
    y = torch.empty_like(x)
    entry, what = _wide_entry("conv_b", rb)
    _lib.check(entry(_p(a), _p(x), _p(rb["wb"]), _p(rb["bb"]), _p(y), B, T, H, W, C, s), what)
    return y


def res(x, cin, emb, rb, bk, s):
    """One ResBlock: x, the cache entry cin or None, the address emb of the FiLM scale | shift (a wide block takes None for none)
    -> (x + conv B(u), the new cache entry).  Two launches, or where bk["wide"] four: act, conv A, act, conv B."""
    if not bk.get("wide"):
        u, cout = res_a(x, cin, emb, rb, bk, s)
        return res_b(u, x, rb, bk, s), cout
    seq, cout = wide_act(x, s, emb, cin, bk["g"])
    u = wide_conv_a(seq, rb, bk["g"], s)
    a2, _ = wide_act(u, s, out=seq.view(-1)[:x.numel()].view(x.shape))    # S is free again: SiLU(RMS(a)) goes there
    return wide_conv_b(a2, x, rb, s), cout


def out(x, bk, s, lvm=None, want="next"):
    """oniris_vae_out, or oniris_vae_wide_out where bk["wide"]: x (B, T, H, W, C) -> by `want` "next": the next block's input
    (B, T, H, W, Cout); "moments": (mean, logvar), each (B, Cout / 2, T, H, W); "frames": uint8 (B, T, H, W, Cout / 2).  lvm: the
    logvar multiplier, for the last two."""
    B, T, H, W, C = x.shape
    Cout = bk["Cout"]
    half = 0 if want == "next" else Cout // 2
    y = mean = logvar = frames = None
    if want == "next":
        y = _new(x, B, T, H, W, Cout)
        strides = y.stride()[:4] + (1,)
    elif want == "frames":
        frames = _new(x, B, T, H, W, half, dtype=torch.uint8)
        strides = (0, 0, 0, 0, 0)
    else:
        mean = _new(x, B, half, T, H, W)
        logvar = torch.empty_like(mean)
        sb, sc, st, sh, sw = mean.stride()
        strides = (sb, st, sh, sw, sc)
    entry, what = _wide_entry("out", bk) if bk["wide"] else (_lib.lib.oniris_vae_out, "vae_out")
    _lib.check(entry(_p(x), _p(bk["wo"]), _p(bk["bo"]), B, T, H, W, C, Cout, half, _p(lvm), _p(y if want == "next" else mean),
                     _p(logvar), *strides, _p(frames), s), what)
    return y if want == "next" else frames if want == "frames" else (mean, logvar)


def down(x, strides, dims, normalize, bk, s):
    """oniris_vae_down, or oniris_vae_wide_down where bk["wide_down"]: fp32 or uint8 frames x by `strides` (normalize:
    x / 127.5 - 1 on load) -> (B, T, H, W, C) over `dims`."""
    B, T, H, W = dims
    y = _new(x, B, T, H, W, bk["C"])
    entry, what = _wide_entry("down", bk) if bk.get("wide_down") else (_lib.lib.oniris_vae_down, "vae_down")
    _lib.check(entry(_p(x), int(x.dtype == torch.uint8), *strides, B, T, H, W, bk["Cin"], bk["tc"], bk["sc"], int(normalize),
                     _p(bk["wd"]), _p(bk["bd"]), bk["C"], _p(y), s), what)
    return y


def latents(x, s, mean=None, std=None):
    """oniris_vae_latents: x (B, T, H, W, C) -> the mean (B, C, T, H, W), or, with mean and std, the normalised latents
    (B, T, C, H, W)."""
    B, T, H, W, C = x.shape
    if mean is None:
        y = _new(x, B, C, T, H, W)
        sb, sc, st, sh, sw = y.stride()
    else:
        y = _new(x, B, T, C, H, W)
        sb, st, sc, sh, sw = y.stride()
    _lib.check(_lib.lib.oniris_vae_latents(_p(x), B, T, H, W, C, _p(mean), _p(std), _p(y), sb, st, sh, sw, sc, s), "vae_latents")
    return y


class GroupCausal3DConvVAE(nn.Module):
    """Parameter holder with the reference's layout (vae.py:18-34): conv3d (C g, C, 2g, 3, 3), stride g in time."""

    def __init__(self, in_channels, out_channels, kernel, group_size):
        super().__init__()
        self.out_channels, self.group_size = out_channels, group_size
        self.conv3d = nn.Conv3d(in_channels, out_channels * group_size, kernel, stride=(group_size, 1, 1), bias=True)
        with torch.no_grad():
            w = self.conv3d.weight
            w[:, :, :-group_size] = 0
            self.conv3d.weight.copy_(w * 32 ** -.25)
        self.register_buffer("group_size_tensor", torch.tensor(group_size), persistent=False)


class ResBlock(nn.Module):
    """vae.py:56-93 (parameters only; the computation is oniris_vae_res_a / oniris_vae_res_b)."""

    def __init__(self, channels, kernel, group_size=1, t_cond=False):
        super().__init__()
        self.conv3d0 = GroupCausal3DConvVAE(channels, channels, kernel, group_size)
        self.conv3d1 = nn.Conv3d(channels, channels, kernel_size=(1, 3, 3), padding=(0, 1, 1))
        nn.init.zeros_(self.conv3d1.weight)
        nn.init.zeros_(self.conv3d1.bias)
        if t_cond:
            self.fourier_cond = MPFourier(channels * 2)
            self.t_cond = nn.Linear(channels * 2, channels * 2)
            nn.init.zeros_(self.t_cond.weight)
            nn.init.zeros_(self.t_cond.bias)


class EncoderDecoderBlock(nn.Module):
    """vae.py:96-133 (parameters only)."""

    def __init__(self, in_channels, out_channels, time_compression, spatial_compression, kernel, group_size, n_res_blocks,
                 type="encoder"):
        super().__init__()
        self.time_compression, self.spatial_compression = int(time_compression), int(spatial_compression)
        total = self.time_compression * self.spatial_compression ** 2
        dec = type == "decoder"
        self.decompression_block = nn.Conv3d(in_channels, in_channels * total, kernel_size=(1, 1, 1)) if dec else None
        self.compression_block = None if dec else nn.Conv3d(in_channels * total, out_channels, kernel_size=(1, 1, 1))
        self.res_blocks = nn.ModuleList([ResBlock(in_channels if dec else out_channels, kernel, group_size, t_cond=dec)
                                         for _ in range(n_res_blocks)])
        self.final_conv = nn.Conv3d(in_channels, out_channels, kernel_size=(1, 1, 1)) if dec else None


class EncoderDecoder(nn.Module):
    """vae.py:167-204 (parameters only): the decoder reverses `channels`, doubles its last entry (mean | logvar) and keeps the
    group sizes cumprod(time_compressions) in order."""

    def __init__(self, channels, n_res_blocks, time_compressions, spatial_compressions, type):
        super().__init__()
        assert type in ["encoder", "decoder"], "Invalid type, expected encoder or decoder"
        assert len(channels) - 1 == len(time_compressions) == len(spatial_compressions)
        self.time_compressions, self.spatial_compressions, self.encoding_type = time_compressions, spatial_compressions, type
        channels = list(channels)
        group_sizes = np.cumprod(time_compressions)
        if type == "encoder":
            group_sizes = group_sizes[::-1]
        else:
            channels = channels[::-1]
            self.logvar_multiplier = nn.Parameter(torch.tensor(-2.))
            channels[-1] = channels[-1] * 2
        self.in_channels, self.out_channels = channels[:-1], channels[1:]
        self.group_sizes = [int(g) for g in group_sizes]
        self.encoder_blocks = nn.ModuleList([
            EncoderDecoderBlock(self.in_channels[i], self.out_channels[i], time_compressions[i], spatial_compressions[i],
                                (self.group_sizes[i] * 2, 3, 3), self.group_sizes[i], n_res_blocks, type)
            for i in range(len(group_sizes))])


class VAE(BetterModule):
    """The reference's VAE (vae.py:207-318) on HIP kernels.  Supported: every block width <= 256 with at most 64 latent
    channels, time and spatial compressions in {1, 2}, any n_res_blocks, any latent height / width; anything else raises
    NotImplementedError here.  Blocks of up to 64 channels run on the register-tile kernels (csrc/vae.hip, csrc/vae_encoder.hip),
    wider ones on the fp32 MFMA tile kernels (csrc/vae_wide.hip), encoder and decoder alike; a model may mix them.  A model
    with a width above 64 runs for inference only unless `wide_training()` was called on it: until then the training path of
    `forward` raises NotImplementedError.  512 channels, the full-size Counter-Strike VAE, are refused here and run through
    `VAE512`, the same model with max_width = 512."""

    max_width = MAX_WIDTH               # the widest block the constructor accepts (VAE512: 512)
    _wide_training_default = False      # the training path of a model with a wide block, as constructed (VAE512: on)

    def __init__(self, channels, n_res_blocks, time_compressions=[1, 2, 2], spatial_compressions=[1, 2, 2], mean=None, std=None):
        super().__init__()
        if len(channels) - 1 != len(time_compressions) or len(channels) - 1 != len(spatial_compressions) or len(channels) < 2:
            raise ValueError("VAE: len(channels) - 1 must equal the number of time and spatial compressions")
        widths = list(channels[::-1][:-1])
        if max(widths) > self.max_width or min(widths) < 1:
            raise NotImplementedError(f"VAE decoder: block widths {widths}: the HIP kernels take 1..{self.max_width} channels")
        if any(int(c) not in (1, 2) for c in list(time_compressions) + list(spatial_compressions)):
            raise NotImplementedError(f"VAE decoder: compressions {list(time_compressions)} / {list(spatial_compressions)}: "
                                      "the HIP kernels take 1 or 2")
        if channels[-1] > MAX_NARROW:
            raise NotImplementedError(f"VAE decoder: {channels[-1]} latent channels: the first block reads the strided latents "
                                      f"on the narrow kernels, which take 1..{MAX_NARROW} channels")
        self.latent_channels = channels[-1]
        self._wide = max(widths) if max(widths) > MAX_NARROW else 0
        self._wide_training = self._wide_training_default
        self._bf16_inference = False
        self.encoder = EncoderDecoder(channels, n_res_blocks, time_compressions, spatial_compressions, type="encoder")
        self.decoder = EncoderDecoder(channels, n_res_blocks, time_compressions, spatial_compressions, type="decoder")
        self.time_compression = np.prod(time_compressions)
        self.spatial_compression = np.prod(spatial_compressions)
        if mean is not None:
            self.register_buffer("mean", torch.tensor(mean), persistent=False)
            self.register_buffer("std", torch.tensor(std), persistent=False)
        frame = inspect.currentframe()
        args, _, _, values = inspect.getargvalues(frame)
        self.kwargs = {arg: values[arg] for arg in args if arg != "self"}

    def wide_training(self, enabled=True):
        """Switch the training path of `forward` on (or off again) for a model with a block wider than MAX_NARROW: the backward on
        the fp32 MFMA kernels of csrc/vae_wide_train.hip (vae_train.py).  Off by default, so that a wide model refuses to train as
        it always has until asked: `VAE.from_pretrained(path).to("cuda").wide_training()` (VAE512 is constructed with it on).  A plain attribute: copy.deepcopy keeps
        it, state_dict and kwargs do not hold it.  A model without a wide block trains either way, on the same kernels.  Returns
        self."""
        self._wide_training = bool(enabled)
        return self

    def bf16_inference(self, enabled=True):
        """Switch the bf16-operand inference kernels (csrc/vae_wide_bf16.hip) on (or off again) for the blocks wider than MAX_NARROW:
        `VAE512.from_pretrained(path).to("cuda").eval().bf16_inference()`.  Off as constructed, for `VAE` and `VAE512` alike.

        The contract (csrc/vae_wide_bf16.h).  While it is on, in a wide block the two operands of every matrix product -- conv A,
        conv B, `up`, `down`, `out`, and the GEMM `down` of a narrow block that compresses more than MAX_DOWN_K channels, the one other
        MFMA launch of the VAE -- are rounded to bf16, round-to-nearest-even, exactly once: the weights when they are packed
        (`weight.to(torch.bfloat16)`), the activated input while a kernel stages it.  Everything else stays fp32: the accumulation
        (in an order fixed by (C, g, tc, sc, Cout) alone, so the bit identities of chunked decoding and encoding hold as before),
        the bias, the residual x of conv B and the channel-area residuals of `out` and `down` (read from the unrounded tensor),
        exp(logvar_multiplier), the uint8 conversion, the activation pass, the t-embedding, every tensor between launches and
        every cache entry: a cache written in one mode is accepted in the other.  The register-tile kernels of the narrow blocks
        (csrc/vae.hip, csrc/vae_conv3.h, csrc/vae_encoder.hip) are untouched.

        It governs `encode`, `encode_long_sequence`, `encode_frames`, `frames_to_latents`, `decode`, `decode_frames`,
        `latents_to_frames`, and `forward` in eval mode or under torch.no_grad().  The training path of `forward` ignores it: it stays
        fp32 and keeps its bits (it packs fp32 weights of its own; a model that alternates training steps and bf16 inference
        re-packs at every change of side).  The packs are rebuilt when the switch changes; with it on a wide block's pack holds the
        bf16 weights and no fp32 copy of them.  A plain attribute like `wide_training`: copy.deepcopy keeps it, state_dict and
        kwargs do not hold it.  On a model without a wide block it is accepted and changes nothing.  Returns self."""
        self._bf16_inference = bool(enabled)
        return self

    # ---- encode + mix + decode (vae.py:228-237)
    def forward(self, x, t=0.1, cache=None, *, t_sample=None, noise=None):
        """x (B, 3, T, H, W) in [-1, 1] -> (r_mean, r_logvar, mean, cache): mean = encode(x), t_b = rand(B) t,
        z = mean (1 - t_b) + randn_like(mean) t_b, (r_mean, r_logvar) = decode(z, t_b); cache = {"encoder": ..., "decoder": ...}.
        t_sample (B,) replaces rand(B) t and noise (the shape of mean) replaces randn_like(mean) (reproducible draws, like the
        sampler's noise= / churn_noise=); otherwise they are drawn on x.device in the reference's order.

        In training mode with grad enabled this is the differentiable path (vae_train.py, csrc/vae_train.hip): the three outputs
        carry a grad_fn, and a loss on them followed by .backward() fills .grad of every VAE parameter that requires grad.  As in
        the reference's training mode, the time prefix of every group-causal conv is the first g activated input frames,
        detached, and every leaf of the returned cache is None; a cache with tensors in it raises ValueError (training through a
        carried cache is not supported), and so does an x that requires grad (frames are data: no gradient is produced for them).

        In eval mode or under torch.no_grad() it is encode -> mix -> decode on the inference kernels: real caches are carried
        under cache["encoder"] / cache["decoder"] and the outputs have no grad_fn.  A model with a block wider than MAX_NARROW has
        this path only, and its training path raises NotImplementedError that names the width, until `wide_training()` switches
        its training path on: then everything said above holds for it too (csrc/vae_wide_train.hip)."""
        self._check_frames("forward", x.shape, "x (B, {c}, T, H, W)", *(x.shape if x.dim() == 5 else (None,) * 5))
        if self._wide:                                       # said before anything else is looked at, wherever the model lives
            self._encoder_device("forward", x)
            if self.training and torch.is_grad_enabled() and not self.__dict__.get("_wide_training", False):
                raise NotImplementedError(f"VAE.forward: this model has a block of {self._wide} channels: above {MAX_NARROW} the "
                                          f"encoder and decoder run for inference only (eval mode or torch.no_grad()); for "
                                          f"training at that width use {_REF}.  VAE.wide_training() switches the fp32 MFMA "
                                          f"training kernels on for this model")
        B = x.shape[0]
        if t_sample is not None and (t_sample.dim() != 1 or t_sample.shape[0] != B):
            raise ValueError(f"VAE.forward: t_sample must be ({B},), got {tuple(t_sample.shape)}")
        lat = (B, self.latent_channels, x.shape[2] // int(self.time_compression), x.shape[3] // int(self.spatial_compression),
               x.shape[4] // int(self.spatial_compression))
        if noise is not None and tuple(noise.shape) != lat:
            raise ValueError(f"VAE.forward: noise must have the shape of mean {lat}, got {tuple(noise.shape)}")
        dev = self._encoder_device("forward", x)
        training = self.training and torch.is_grad_enabled()
        cache = {} if cache is None else cache
        if training and x.requires_grad:
            raise ValueError("VAE.forward: x requires grad, but no gradient with respect to the frames is produced")
        if training and _has_tensor(cache):
            raise ValueError("VAE.forward: a non-empty cache on the training path (training through a carried cache is not supported)")
        t_b = (torch.rand(B, device=dev, dtype=torch.float32) * t if t_sample is None
               else t_sample.detach().to(device=dev, dtype=torch.float32))
        if noise is not None:
            noise = noise.detach().to(device=dev, dtype=torch.float32)
        if training:
            from . import vae_train
            r_mean, r_logvar, mean = vae_train.run(self, x, t_b, noise)
            leaves = lambda ed: {f"encoder_block_{i}": {f"res_block_{j}": {"conv3d_res0": None} for j in range(len(blk.res_blocks))}
                                 for i, blk in enumerate(ed.encoder_blocks)}
            return r_mean, r_logvar, mean, {"encoder": leaves(self.encoder), "decoder": leaves(self.decoder)}
        with torch.no_grad():
            mean, enc_cache = self.encode(x, cache.get("encoder"))
            if noise is None:
                noise = torch.randn_like(mean)
            z = bmult(mean, 1 - t_b) + bmult(noise, t_b)
            r_mean, r_logvar, dec_cache = self.decode(z, t_b, cache.get("decoder"))
        return r_mean, r_logvar, mean, {"encoder": enc_cache, "decoder": dec_cache}

    # ---- packed device weights
    def _pack(self, device, bf16=None):
        """fp32 device copies of the decoder's parameters in the layouts of csrc/vae.hip and vae_conv3.h, rebuilt when one changed.
        bf16 (None: as `bf16_inference` set it; the training path passes False): the weights of the wide blocks as bf16
        (csrc/vae_wide_bf16.h); part of the signature, so a change rebuilds the pack."""
        bf16 = bool(self.__dict__.get("_bf16_inference", False) if bf16 is None else bf16)
        params = list(self.decoder.parameters()) + list(self.decoder.buffers())
        sig = (str(device), bf16) + tuple((p.data_ptr(), p._version) for p in params)
        pk = self.__dict__.get("_oniris_vae_pack")
        if pk is not None and pk["sig"] == sig:
            return pk
        f32 = dict(device=device, dtype=torch.float32)
        blocks, tparams, table, eoff = [], [], [], 0
        with torch.no_grad():
            for i, blk in enumerate(self.decoder.encoder_blocks):
                C, Cout, g = self.decoder.in_channels[i], self.decoder.out_channels[i], self.decoder.group_sizes[i]
                wide = C > MAX_NARROW
                nch, gpt = (0, 0) if wide else (_nch(C), _gpt(C, g))
                res = []
                for rb in blk.res_blocks:
                    res.append(dict(_pack_res_wide(rb, C, g, f32, bf16) if wide else _pack_res(rb, C, g, f32), emb_off=eoff))
                    off = sum(x.numel() for x in tparams)
                    tparams += [rb.fourier_cond.freqs.detach().to(**f32), rb.fourier_cond.phases.detach().to(**f32),
                                rb.t_cond.weight.detach().to(**f32).reshape(-1), rb.t_cond.bias.detach().to(**f32)]
                    table += [off, 2 * C, eoff]
                    eoff += 2 * C
                bk = dict(C=C, Cout=Cout, g=g, nch=nch, gpt=gpt, tc=blk.time_compression, sc=blk.spatial_compression, wide=wide,
                          wu=blk.decompression_block.weight.detach().to(**f32).reshape(-1, C).contiguous(),
                          bu=blk.decompression_block.bias.detach().to(**f32).contiguous(),
                          wo=blk.final_conv.weight.detach().to(**f32).reshape(Cout, C).contiguous(),
                          bo=blk.final_conv.bias.detach().to(**f32).contiguous(), res=res)
                if wide:                                             # the 1x1 stages as GEMMs (csrc/vae_wide_conv.h)
                    bk["wu"], bk["bu"] = _pack_lin_wide(blk.decompression_block.weight, blk.decompression_block.bias, C, C,
                                                        blk.time_compression * blk.spatial_compression ** 2, f32, bf16)
                    bk["wo"], bk["bo"] = _pack_lin_wide(blk.final_conv.weight, blk.final_conv.bias, C, Cout, 1, f32, bf16)
                    if bf16:
                        bk["bf16"] = True
                blocks.append(bk)
            pk = dict(sig=sig, blocks=blocks, tparams=torch.cat(tparams).contiguous(),
                      table=torch.tensor(table, dtype=torch.int32, device=device), n_rb=len(table) // 3, emb_per_row=eoff,
                      lvm=self.decoder.logvar_multiplier.detach().to(**f32).reshape(1).contiguous())
        self.__dict__["_oniris_vae_pack"] = pk
        return pk

    # ---- the ResBlocks of one block, for both sides
    @staticmethod
    def _res_blocks(side, i, bk, x, cache, emb_of, s):
        """x (B, T, H, W, C) through the ResBlocks of packed block bk (block i of `side`) with the block's entry of the incoming
        cache; emb_of(rb): the address of a ResBlock's FiLM scale | shift.  Returns (x, the block's entry of the new cache)."""
        B, T, H, W, C = x.shape
        g, new_cache = bk["g"], {}
        for j, rb in enumerate(bk["res"]):
            cin = cache.get(f"res_block_{j}", {}).get("conv3d_res0")
            if cin is not None and (tuple(cin.shape) != (B, g, H, W, C) or cin.device != x.device or cin.dtype != torch.float32):
                raise ValueError(f"VAE {side} cache entry encoder_block_{i}.res_block_{j} has shape {tuple(cin.shape)}, "
                                 f"expected {(B, g, H, W, C)} (a cache from another batch or resolution)")
            x, cout = res(x, cin, emb_of(rb), rb, bk, s)
            new_cache[f"res_block_{j}"] = {"conv3d_res0": cout}
        return x, new_cache

    # ---- the decoder
    def _run(self, x, strides, t, cache, in_affine=False, want="moments"):
        """x: latents addressed by element strides (b, t, h, w, c); returns ((mean, logvar) | frames, cache)."""
        B, T, h, w_ = x.shape[0], x.shape[1 if want == "frames" else 2], x.shape[-2], x.shape[-1]
        dev = x.device
        if dev.type != "cuda":
            raise RuntimeError("VAE decoder: the latents must be on the GPU (the decoder runs on HIP kernels only)")
        pk = self._pack(dev)
        s = _stream()
        t = torch.as_tensor(t, dtype=torch.float32, device=dev)
        t = (t.expand(B) if t.dim() == 0 else t.reshape(B)).contiguous()
        emb = temb(pk, self._wide, t, s)
        cache = {} if cache is None else cache
        new_cache = {}
        scale = shift = None
        if in_affine:
            if not hasattr(self, "mean"):
                raise RuntimeError("VAE: latents_to_frames needs the `mean` / `std` constructor arguments (as in the reference)")
            scale = self.std.to(device=dev, dtype=torch.float32).contiguous()
            shift = self.mean.to(device=dev, dtype=torch.float32).contiguous()
        H, W = h, w_
        nblk = len(pk["blocks"])
        for i, bk in enumerate(pk["blocks"]):
            # a wide block is never block 0: its x is the contiguous output of the block before
            x = up(x, strides, (B, T, H, W), bk, s, scale, shift)
            T, H, W = x.shape[1:4]
            scale = shift = None
            x, new_cache[f"encoder_block_{i}"] = self._res_blocks("decoder", i, bk, x, cache.get(f"encoder_block_{i}", {}),
                                                                  lambda rb: emb.data_ptr() + 4 * B * rb["emb_off"], s)
            if i < nblk - 1:
                x = out(x, bk, s)
                strides = x.stride()[:4] + (1,)
            else:
                return out(x, bk, s, pk["lvm"], want), new_cache

    @torch.no_grad()
    def decode(self, z, t, cache=None):
        """z (B, C, T, h, w) -> (mean, logvar, cache), mean / logvar (B, 3, 4T, 4h, 4w) (vae.py:253-255).  The cache holds, under
        the reference's keys cache['encoder_block_{i}']['res_block_{j}']['conv3d_res0'], the last g activated input frames of
        every group-causal conv as opaque channels-last (B, g, H, W, C) fp32 tensors; pass it back to continue the sequence."""
        if z.dim() != 5 or z.shape[1] != self.latent_channels:
            raise ValueError(f"VAE.decode: z must be (B, {self.latent_channels}, T, h, w), got {tuple(z.shape)}")
        z = z.float()
        sb, sc, st, sh, sw = z.stride()
        (mean, logvar), cache = self._run(z, (sb, st, sh, sw, sc), t, cache)
        return mean, logvar, cache

    @torch.no_grad()
    def decode_frames(self, latents, t=0.1, cache=None):
        """Streaming latents_to_frames: latents (B, t, C, h, w) (normalised, as the sampler returns them) -> (frames (B, 4t, H, W, 3)
        uint8 on the device, cache).  Feed the returned cache to the next call: frame by frame, the result equals
        latents_to_frames over the whole sequence."""
        if latents.dim() != 5 or latents.shape[2] != self.latent_channels:
            raise ValueError(f"VAE.decode_frames: latents must be (B, t, {self.latent_channels}, h, w), got {tuple(latents.shape)}")
        latents = latents.float()
        sb, st, sc, sh, sw = latents.stride()
        return self._run(latents, (sb, st, sh, sw, sc), t, cache, in_affine=True, want="frames")

    @torch.no_grad()
    def latents_to_frames(self, latents, t=0.1):
        """latents (B, T, C, h, w) -> numpy int array (B, 4T, H, W, 3) = clip((mean + 1) 127.5, 0, 255) truncated (vae.py:288-318)."""
        frames, _ = self.decode_frames(latents, t)
        return frames.cpu().numpy().astype(int)

    # ---- the encoder
    def _pack_encoder(self, device, bf16=None):
        """fp32 copies of the encoder's parameters on `device` in the layouts of csrc/vae_encoder.hip and csrc/vae_conv3.h, rebuilt
        when a parameter changed.  pk["params"] names every state_dict entry that went into it.  A block wider than MAX_NARROW
        carries wide=True and its ResBlocks the layouts of csrc/vae_wide_conv.h; its `down`, and that of any block compressing
        more than MAX_DOWN_K channels, carries wide_down=True and the GEMM layout (_pack_down_wide).  Every other block holds
        exactly what it held before there were wide ones.  bf16: as in _pack; the ResBlocks of a wide block then hold bf16 weights
        and bf16=True, and so does every block whose `down` is the GEMM (wide_down: an MFMA launch, whatever the block's width)."""
        bf16 = bool(self.__dict__.get("_bf16_inference", False) if bf16 is None else bf16)
        params = list(self.encoder.parameters())
        sig = (str(device), bf16) + tuple((p.data_ptr(), p._version) for p in params)
        pk = self.__dict__.get("_oniris_vae_enc_pack")
        if pk is not None and pk["sig"] == sig:
            return pk
        f32 = dict(device=device, dtype=torch.float32)
        blocks, names = [], []
        with torch.no_grad():
            for i, blk in enumerate(self.encoder.encoder_blocks):
                Cin, C, g = self.encoder.in_channels[i], self.encoder.out_channels[i], self.encoder.group_sizes[i]
                npos = blk.time_compression * blk.spatial_compression ** 2
                K = Cin * npos
                wide, wide_down = C > MAX_NARROW, C > MAX_NARROW or K > MAX_DOWN_K
                if wide_down:                                  # the GEMM of csrc/vae_wide_conv.h
                    wd, bd = _pack_down_wide(blk.compression_block.weight, blk.compression_block.bias, Cin, C, npos, f32, bf16)
                else:
                    g4 = (C + 3) // 4 * 4
                    wd = torch.zeros(K, 2, g4, **f32)          # per k = ((tc hc) wc) c: the conv weights | the area windows
                    wd[:, 0, :C] = blk.compression_block.weight.detach().to(**f32).reshape(C, K).t()
                    bd = torch.ones(2, g4, **f32)              # the bias | the window lengths
                    bd[0] = 0
                    bd[0, :C] = blk.compression_block.bias.detach().to(**f32)
                    for o, (s0, s1) in enumerate(_area_windows(K, C)):
                        wd[s0:s1, 1, o] = 1
                        bd[1, o] = s1 - s0
                pre = f"encoder.encoder_blocks.{i}."
                names += [pre + "compression_block.weight", pre + "compression_block.bias"]
                res = []
                for j, rb in enumerate(blk.res_blocks):
                    res.append(_pack_res_wide(rb, C, g, f32, bf16) if wide else _pack_res(rb, C, g, f32))
                    names += [pre + f"res_blocks.{j}.{n}" for n in ("conv3d0.conv3d.weight", "conv3d0.conv3d.bias", "conv3d1.weight",
                                                                   "conv3d1.bias")]
                nch, gpt = (0, 0) if wide else (_nch(C), _gpt(C, g))
                bk = dict(Cin=Cin, C=C, g=g, nch=nch, gpt=gpt, tc=blk.time_compression, sc=blk.spatial_compression,
                          wd=wd.contiguous(), bd=bd, res=res)
                if wide:
                    bk["wide"] = True
                if wide_down:
                    bk["wide_down"] = True
                    if bf16:                                   # read by `down` alone: a ResBlock's pack carries its own flag
                        bk["bf16"] = True
                blocks.append(bk)
            pk = dict(sig=sig, blocks=blocks, params=names, zeros={})
        self.__dict__["_oniris_vae_enc_pack"] = pk
        return pk

    def _check_frames(self, what, shape, layout, B, C, T, H, W):
        """The shape checks of every encoder entry point; they come before anything else."""
        tcomp, scomp, c0 = int(self.time_compression), int(self.spatial_compression), self.encoder.in_channels[0]
        if B is None or C != c0:
            raise ValueError(f"VAE.{what}: expected {layout.format(c=c0)}, got {tuple(shape)}")
        if T % tcomp != 0 or T == 0:
            raise ValueError(f"VAE.{what}: {T} frames: the number of frames must be a positive multiple of the time compression {tcomp}")
        if H % scomp != 0 or W % scomp != 0 or H == 0 or W == 0:
            raise ValueError(f"VAE.{what}: frames of {H} x {W}: height and width must be positive multiples of the spatial "
                             f"compression {scomp}")

    def _check_groups(self, T):
        """Block i sees T / (its cumulative time compression) frames in groups of g_i, and every group must be whole; the default
        compressions ask for no more than _check_frames does.  Said once the model is known to run (after the device check)."""
        need = 1
        for i in range(len(self.encoder.encoder_blocks)):
            need = int(np.lcm(need, self.encoder.group_sizes[i] * int(np.prod(self.encoder.time_compressions[:i + 1]))))
        if T % need != 0:
            raise ValueError(f"VAE encoder: {T} frames: with time compressions {list(self.encoder.time_compressions)} every block must "
                             f"see whole groups of frames (group sizes {self.encoder.group_sizes}), so the number of frames, of a "
                             f"chunk too, must be a multiple of {need} (as in the reference)")

    def _encoder_device(self, what, x=None):
        """The device the encoder runs on; a model or an input on the CPU is refused, after the shape checks and before anything is
        packed or launched.  A model with a block wider than MAX_NARROW says so: its refusal names the widest width."""
        dev = self.device if x is None else x.device
        if (dev.type != "cuda" or self.device.type != "cuda") and self._wide:
            raise NotImplementedError(f"VAE.{what}: this model has a block of {self._wide} channels: the encoder and the decoder at "
                                      f"that width run on HIP kernels only (model and input on the GPU); on the CPU use {_REF}")
        if dev.type != "cuda" or self.device.type != "cuda":
            raise NotImplementedError(f"VAE.{what}: the encoder runs on HIP kernels only (model and input on the GPU); on the CPU "
                                      f"use {_REF}")
        return dev

    def _run_enc(self, x, strides, T, H, W, normalize, cache, want="mean"):
        """x: fp32 or uint8 frames addressed by element strides (b, t, h, w, c); returns (mean (B, C, t, h, w) | normalised latents
        (B, t, C, h, w), cache)."""
        B, dev = x.shape[0], x.device
        self._check_groups(T)
        pk = self._pack_encoder(dev)
        s = _stream()
        zeros = pk["zeros"].get(B)
        if zeros is None:                                    # the FiLM scale | shift of a ResBlock without t: zero
            zeros = pk["zeros"][B] = torch.zeros(B * 2 * max(MAX_WIDTH, self._wide), dtype=torch.float32, device=dev)
        cache = {} if cache is None else cache
        new_cache = {}
        for i, bk in enumerate(pk["blocks"]):
            T, H, W = T // bk["tc"], H // bk["sc"], W // bk["sc"]
            x = down(x, strides, (B, T, H, W), normalize, bk, s)
            strides, normalize = x.stride()[:4] + (1,), False
            # a wide block's activation pass takes a null FiLM pointer
            x, new_cache[f"encoder_block_{i}"] = self._res_blocks("encoder", i, bk, x, cache.get(f"encoder_block_{i}", {}),
                                                                  lambda rb: None if bk.get("wide") else _p(zeros), s)
        if want == "latents":
            return latents(x, s, self.mean.to(device=dev, dtype=torch.float32).contiguous(),
                           self.std.to(device=dev, dtype=torch.float32).contiguous()), new_cache
        return latents(x, s), new_cache

    @torch.no_grad()
    def encode(self, x, cache=None):
        """x (B, 3, T, H, W) in [-1, 1] -> (mean (B, C, T / 4, H / 4, W / 4), cache) (vae.py:239-241).  The cache holds, under the
        reference's keys cache['encoder_block_{i}']['res_block_{j}']['conv3d_res0'], the last g activated input frames of every
        group-causal conv as opaque channels-last (B, g, H, W, C) fp32 tensors; pass it back to continue the sequence."""
        self._check_frames("encode", x.shape, "x (B, {c}, T, H, W)", *(x.shape if x.dim() == 5 else (None,) * 5))
        self._encoder_device("encode", x)
        x = x.float()
        sb, sc, st, sh, sw = x.stride()
        return self._run_enc(x, (sb, st, sh, sw, sc), x.shape[2], x.shape[3], x.shape[4], False, cache)

    @torch.no_grad()
    def encode_long_sequence(self, frames, cache=None, split_size=256):
        """encode over chunks of split_size frames through the cache, each moved to the model's device on its own; returns the
        mean (vae.py:250-259).  split_size must be a multiple of the time compression."""
        self._check_frames("encode_long_sequence", frames.shape, "frames (B, {c}, T, H, W)",
                           *(frames.shape if frames.dim() == 5 else (None,) * 5))
        if split_size <= 0 or split_size % int(self.time_compression) != 0:
            raise ValueError(f"VAE.encode_long_sequence: split_size {split_size} must be a positive multiple of the time compression "
                             f"{int(self.time_compression)}")
        dev = self._encoder_device("encode_long_sequence")
        means = []
        for s0 in range(0, frames.shape[2], split_size):
            m, cache = self.encode(frames[:, :, s0:s0 + split_size].to(dev), cache=cache)
            means.append(m)
        return torch.cat(means, dim=2)

    @torch.no_grad()
    def encode_frames(self, frames, cache=None):
        """Streaming frames_to_latents: frames (B, 4t, H, W, 3) with values 0..255, uint8 or any real dtype, on the GPU ->
        (latents (B, t, C, h, w) fp32, normalised as Precond and the sampler take them, cache).  uint8 frames are read in place and
        frames / 127.5 - 1 is applied on load.  Feed the returned cache to the next call: chunk by chunk (the smallest chunk is one
        latent frame; two where a time compression of 1 follows one of 2, as in channels=[3,16,64,256,8]: every block must see
        whole groups), the result equals frames_to_latents over the whole sequence."""
        B, T, H, W, C = frames.shape if frames.dim() == 5 else (None,) * 5
        self._check_frames("encode_frames", frames.shape, "frames (B, T, H, W, {c})", B, C, T, H, W)
        self._encoder_device("encode_frames", frames)
        if not hasattr(self, "mean"):
            raise RuntimeError("VAE: frames_to_latents needs the `mean` / `std` constructor arguments (as in the reference)")
        if frames.dtype != torch.uint8:
            frames = frames.float()
        sb, st, sh, sw, sc = frames.stride()
        return self._run_enc(frames, (sb, st, sh, sw, sc), T, H, W, True, cache, want="latents")

    @torch.no_grad()
    def frames_to_latents(self, frames):
        """frames (B, T, H, W, 3), values 0..255 -> latents (B, T / 4, C, h, w) = (encode(frames / 127.5 - 1) - mean) / std, the
        formula cs_train.py:102 applies by hand and the inverse of the affine in latents_to_frames.  (The reference's own method,
        vae.py:264-284, does not run: it unpacks four values from encode, adds std and returns nothing.)"""
        return self.encode_frames(frames)[0]


class VAE512(VAE):
    """`VAE` for block widths up to 512 channels: the full-size Counter-Strike VAE, channels=[3, 32, 128, 512, 8] with
    n_res_blocks=5, time_compressions=[1, 2, 2, 1] and spatial_compressions=[1, 2, 2, 2] (cs_vae_train.py:34-39).  The same
    constructor, `kwargs`, state_dict keys, checkpoint format, cache keys, methods and ValueErrors: `from
    autoregressive_diffusion_amd.vae import VAE512 as VAE` is the whole change on the user's side, and
    `VAE512.from_pretrained(path)` loads what `VAE` or the reference wrote (and `VAE` what this class wrote, up to 256 channels).
    Two differences: a width above 512 (not 256) raises NotImplementedError, and the training path of `forward` is on as
    constructed; `wide_training(False)` still turns it off.  More than 64 latent channels and compressions other than 1 or 2 are
    refused as in `VAE`.  A model whose widest block has at most 256 channels runs the launches of `VAE(...).wide_training()`,
    bit for bit.  The kernels are those of csrc/vae_wide.hip and csrc/vae_wide_train.hip, which never bounded the width; what a
    block above 256 channels changes is the weight-gradient workspace (vae_train._nslab) and the activation adjoint's
    instantiation (csrc/vae_wide_train.h)."""

    max_width = 512
    _wide_training_default = True
