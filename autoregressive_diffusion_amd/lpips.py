"""LPIPS, the perceptual loss of the VAE's training loop (reference: cs_vae_train.py:80-82,118, cs_vae_adversarial.py:91-93,126) --
`from autoregressive_diffusion_amd.lpips import LPIPS` in place of `lpips.LPIPS`, with the weights of the `lpips` package handed over:

    lpips_loss_fn = LPIPS(net='alex', weights=lpips.LPIPS(net='alex').state_dict())

The `lpips` package is never imported here.  With fp32 GPU operands the AlexNet trunk, the unit-normalised feature differences and
the 1x1 heads run on HIP kernels, forward and backward (include/oniris.h: oniris_lpips_*, csrc/lpips.hip, csrc/lpips_conv.h): the two
operands pass the trunk as one channels-last batch of 2 N images, the stride-1 convs and their data gradients are one fp32
implicit-GEMM kernel on the exact-f32 matrix instruction, ReLU is an epilogue, the max-pool adjoint is a gather.  No atomics: two
runs give the same bits, and an image's value and gradient do not depend on the images around it.  Every parameter is frozen, so no
weight gradient exists."""
import ctypes

import torch
from torch import nn
from torch.nn import functional as F

from . import _lib
from .vae import _p, _stream

# The state dict of lpips.LPIPS(net='alex'), weights layout 0.1: name -> shape.  Written down from memory of the package: it has NOT
# been verified against an installed copy.  Everything that knows a key name reads this table.
_TRUNK = (("net.slice1.0", 64, 3, 11), ("net.slice2.3", 192, 64, 5), ("net.slice3.6", 384, 192, 3), ("net.slice4.8", 256, 384, 3),
          ("net.slice5.10", 256, 256, 3))
CHANNELS = tuple(t[1] for t in _TRUNK)
KEYS = {"scaling_layer.shift": (1, 3, 1, 1), "scaling_layer.scale": (1, 3, 1, 1)}
for _name, _co, _ci, _k in _TRUNK:
    KEYS[_name + ".weight"] = (_co, _ci, _k, _k)
    KEYS[_name + ".bias"] = (_co,)
for _i, _c in enumerate(CHANNELS):
    KEYS[f"lin{_i}.model.1.weight"] = (1, _c, 1, 1)
    KEYS[f"lins.{_i}.model.1.weight"] = (1, _c, 1, 1)          # the package registers the heads twice: the same tensors
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
MIN_SIZE = 31          # the smallest H, W at which both pools have a window
EPS = 1e-10


def _holder(children):
    m = nn.Module()
    for k, v in children.items():
        m.add_module(k, v)
    return m


def feature_sizes(H, W):
    """The (h, w) of the five feature maps of an H x W image."""
    h1, w1 = (H - 7) // 4 + 1, (W - 7) // 4 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    h3, w3 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
    return [(h1, w1), (h2, w2), (h3, w3), (h3, w3), (h3, w3)]


# ---------------------------------------------------------------------------------------------------------------------------------
# launches: thin wrappers, one per entry point, on channels-last fp32 tensors of the GPU

def _strides(t):
    return (ctypes.c_longlong * 4)(*t.stride())


def pack_conv(w):
    """(Cout, Cin, k, k) -> the forward layout [k k][Cin][Cout] of oniris_lpips_conv."""
    Cout, Cin, k, _ = w.shape
    return w.detach().float().permute(2, 3, 1, 0).reshape(k * k, Cin, Cout).contiguous()


def pack_conv_dgrad(w):
    """(Cout, Cin, k, k) -> the layout of the data gradient: the conv Cout -> Cin on the flipped taps, [k k][Cout][Cin]."""
    Cout, Cin, k, _ = w.shape
    return w.detach().float().flip(2, 3).permute(2, 3, 0, 1).reshape(k * k, Cout, Cin).contiguous()


def pack_stem(w):
    """(64, 3, 11, 11) -> [ky][c][kx][64]."""
    return w.detach().float().permute(2, 1, 3, 0).contiguous()


def pack_stem_dgrad(w):
    """(64, 3, 11, 11) -> [ky][kx][c][64]."""
    return w.detach().float().permute(2, 3, 1, 0).contiguous()


def stem(in0, in1, shift, scale, wp, bias, normalize=False):
    """oniris_lpips_stem: two (N, 3, H, W) operands of any strides -> f1 (2 N, H1, W1, 64)."""
    N, _, H, W = in0.shape
    f1 = torch.empty(2 * N, (H - 7) // 4 + 1, (W - 7) // 4 + 1, 64, dtype=torch.float32, device=in0.device)
    _lib.check(_lib.lib.oniris_lpips_stem(_p(in0), _p(in1), _strides(in0), _strides(in1), N, H, W, int(normalize), _p(shift), _p(scale),
                                          _p(wp), _p(bias), _p(f1), _stream()), "lpips_stem")
    return f1


def stem_dgrad(g1, wd, scale, like, normalize=False):
    """oniris_lpips_stem_dgrad: g1 (NI, H1, W1, 64) -> the gradient of the operand `like` (NI, 3, H, W), in its strides."""
    NI, _, H, W = like.shape
    dx = torch.empty_like(like, memory_format=torch.preserve_format)
    _lib.check(_lib.lib.oniris_lpips_stem_dgrad(_p(g1), _p(wd), _p(scale), NI, H, W, int(normalize), _p(dx), _strides(dx), _stream()),
               "lpips_stem_dgrad")
    return dx


def conv(x, wp, bias, ksize, tile=0):
    """oniris_lpips_conv, mode 0: relu(conv(x) + bias); x (NI, H, W, Cin), wp from pack_conv; tile 0 = chosen by the library."""
    NI, H, W, Cin = x.shape
    Cout = wp.shape[2]
    out = torch.empty(NI, H, W, Cout, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib.oniris_lpips_conv(_p(x), _p(wp), _p(bias), None, None, _p(out), NI, H, W, Cin, Cout, ksize, 0, tile, _stream()),
               "lpips_conv")
    return out


def conv_dgrad(dy, wd, ksize, add=None, f=None, out=None, tile=0):
    """oniris_lpips_conv, mode 1: (conv of dy on the flipped weights + add) * (f > 0); `out` may be `add` itself."""
    NI, H, W, Cin = dy.shape
    Cout = wd.shape[2]
    if out is None:
        out = torch.empty(NI, H, W, Cout, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib.oniris_lpips_conv(_p(dy), _p(wd), None, _p(add), _p(f), _p(out), NI, H, W, Cin, Cout, ksize, 1, tile, _stream()),
               "lpips_conv")
    return out


def pool(x):
    NI, H, W, C = x.shape
    out = torch.empty(NI, (H - 3) // 2 + 1, (W - 3) // 2 + 1, C, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib.oniris_lpips_pool(_p(x), _p(out), NI, H, W, C, _stream()), "lpips_pool")
    return out


def pool_bwd(dp, f, add=None, mask=False, out=None):
    """The adjoint of pool at its input f, (+ add) (* (f > 0)); `out` may be `add` itself."""
    NI, H, W, C = f.shape
    if out is None:
        out = torch.empty_like(f)
    _lib.check(_lib.lib.oniris_lpips_pool_bwd(_p(dp), _p(f), _p(add), int(mask), _p(out), NI, H, W, C, _stream()), "lpips_pool_bwd")
    return out


def heads(feats, ws, N):
    """feats: five (2 N, h, w, C) maps, ws: five [C] head weights -> (N,) the LPIPS distance."""
    dev = feats[0].device
    hw = [f.shape[1] * f.shape[2] for f in feats]
    off, total = [], 0
    for s in hw:
        off.append(total)
        total += N * -(-s // 64)
    part = torch.empty(total, dtype=torch.float32, device=dev)
    for f, w, s, o in zip(feats, ws, hw, off):
        _lib.check(_lib.lib.oniris_lpips_head_fwd(_p(f[:N]), _p(f[N:]), _p(w), _p(part[o:]), N, s, f.shape[3], _stream()),
                   "lpips_head_fwd")
    out = torch.empty(N, dtype=torch.float32, device=dev)
    n = len(feats)
    _lib.check(_lib.lib.oniris_lpips_head_sum(_p(part), n, (ctypes.c_longlong * n)(*off), (ctypes.c_int * n)(*hw), N, _p(out), _stream()),
               "lpips_head_sum")
    return out


def head_bwd(f, w, cot, need0, need1, mask=False):
    """d f of one layer for the operands that need it: (lo .. hi, h, w, C), the slice of the 2 N images that takes a gradient."""
    N = f.shape[0] // 2
    n = (N if need0 else 0) + (N if need1 else 0)
    g = torch.empty((n,) + tuple(f.shape[1:]), dtype=torch.float32, device=f.device)
    ga = g[:N] if need0 else None
    gb = g[n - N:] if need1 else None
    _lib.check(_lib.lib.oniris_lpips_head_bwd(_p(f[:N]), _p(f[N:]), _p(w), _p(cot), _p(ga), _p(gb), int(mask), N, f.shape[1] * f.shape[2],
                                              f.shape[3], _stream()), "lpips_head_bwd")
    return g


# ---------------------------------------------------------------------------------------------------------------------------------
# autograd

class _Distance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, in0, in1, pk, normalize):
        N = in0.shape[0]
        f1 = stem(in0, in1, pk["shift"], pk["scale"], pk["stem"], pk["bias"][0], normalize)
        f2 = conv(pool(f1), pk["fwd"][1], pk["bias"][1], 5)
        f3 = conv(pool(f2), pk["fwd"][2], pk["bias"][2], 3)
        f4 = conv(f3, pk["fwd"][3], pk["bias"][3], 3)
        f5 = conv(f4, pk["fwd"][4], pk["bias"][4], 3)
        feats = [f1, f2, f3, f4, f5]
        out = heads(feats, pk["lin"], N)
        ctx.feats, ctx.pk, ctx.normalize = feats, pk, normalize
        ctx.save_for_backward(in0, in1)
        return out.view(N, 1, 1, 1)

    @staticmethod
    def backward(ctx, dout):
        need0, need1 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need0 or need1):
            return None, None, None, None
        pk, feats = ctx.pk, ctx.feats
        N = feats[0].shape[0] // 2
        lo, hi = (0 if need0 else N), (2 * N if need1 else N)
        cot = dout.reshape(N).float().contiguous()
        g = [head_bwd(f, w, cot, need0, need1, mask=(k == 4)) for k, (f, w) in enumerate(zip(feats, pk["lin"]))]
        f1, f2, f3, f4, _ = [f[lo:hi] for f in feats]
        d4 = conv_dgrad(g[4], pk["bwd"][4], 3, add=g[3], f=f4, out=g[3])
        d3 = conv_dgrad(d4, pk["bwd"][3], 3, add=g[2], f=f3, out=g[2])
        dp2 = conv_dgrad(d3, pk["bwd"][2], 3)
        d2 = pool_bwd(dp2, f2, add=g[1], mask=True, out=g[1])
        dp1 = conv_dgrad(d2, pk["bwd"][1], 5)
        d1 = pool_bwd(dp1, f1, add=g[0], mask=True, out=g[0])
        in0, in1 = ctx.saved_tensors
        dx0 = stem_dgrad(d1[:N], pk["stem_bwd"], pk["scale"], in0, ctx.normalize) if need0 else None
        dx1 = stem_dgrad(d1[d1.shape[0] - N:], pk["stem_bwd"], pk["scale"], in1, ctx.normalize) if need1 else None
        return dx0, dx1, None, None


# ---------------------------------------------------------------------------------------------------------------------------------
# the module

class LPIPS(nn.Module):
    """`lpips.LPIPS(net='alex')`, version 0.1 of its weights layout: forward(in0, in1, normalize=False) -> (N, 1, 1, 1) fp32.

    weights: a state dict, or the path of one saved with torch.save, loaded at once.  Without weights the module holds zeros and
    forward raises RuntimeError until load_state_dict has run: a perceptual loss on random weights must not run silently.  The keys
    are the package's (the table KEYS of this module); a dict that has the heads under only one of `lin{k}` / `lins.{k}` loads too.
    Every parameter is frozen and the module stays in eval behaviour: the package's dropout never applies.

    x <- (x - shift) / scale (normalize=True first maps [0, 1] to [-1, 1]); f1 = relu(conv 11x11 stride 4 pad 2); f2 = relu(conv 5x5
    pad 2 (maxpool 3x3 stride 2 (f1))); f3 = relu(conv 3x3 pad 1 (maxpool 3x3 stride 2 (f2))); f4, f5 = relu(conv 3x3 pad 1); per
    layer n = f / (sqrt(sum_c f^2) + 1e-10) and the layer value is the mean over pixels of sum_c w_c (n0 - n1)^2; the output is the
    sum of the five layer values.

    Native domain: fp32 GPU tensors (N, 3, H, W) of equal shape, H, W >= 31, addressed by element strides -- the (b t) c h w views
    the training scripts make are read in place, and a gradient is written in its operand's strides.  The output is on the autograd
    graph; backward gives the gradient to whichever of in0 / in1 requires it.  Smaller images or operands of different shapes raise
    ValueError.  CPU tensors and other dtypes take `forward_torch`, the same definition as plain torch code.

    One deliberate difference from torch: where every channel of a pixel of a feature map is zero, torch's adjoint of the norm is
    0 / 0 = NaN.  Here that pixel has the unit vector 0 and contributes a zero gradient, in the kernels and in forward_torch."""

    def __init__(self, net="alex", weights=None):
        super().__init__()
        if net != "alex":
            raise NotImplementedError(f"LPIPS: net {net!r}: only 'alex' is built")
        sl = nn.Module()
        sl.register_buffer("shift", torch.tensor(SHIFT).view(1, 3, 1, 1))
        sl.register_buffer("scale", torch.tensor(SCALE).view(1, 3, 1, 1))
        self.scaling_layer = sl
        slices, self._convs = {}, []
        for name, co, ci, k in _TRUNK:
            _, sname, idx = name.split(".")
            c = nn.Conv2d(ci, co, k, stride=4 if k == 11 else 1, padding=2 if k == 11 else k // 2)
            slices[sname] = _holder({idx: c})
            self._convs.append(c)
        self.net = _holder(slices)
        lins = []
        for i, c in enumerate(CHANNELS):
            lin = _holder({"model": _holder({"1": nn.Conv2d(c, 1, 1, bias=False)})})
            self.add_module(f"lin{i}", lin)
            lins.append(lin)
        self.lins = nn.ModuleList(lins)
        for p in self.parameters():
            nn.init.zeros_(p)
            p.requires_grad_(False)
        self._loaded = False
        super().train(False)
        assert set(self.state_dict()) == set(KEYS)
        if weights is not None:
            if not isinstance(weights, dict):
                weights = torch.load(weights, map_location="cpu")
            self.load_state_dict(weights)

    def train(self, mode=True):
        return super().train(False)

    def load_state_dict(self, state_dict, strict=True, **kw):
        sd = dict(state_dict)
        for i in range(len(CHANNELS)):
            a, b = f"lin{i}.model.1.weight", f"lins.{i}.model.1.weight"
            if a in sd and b not in sd:
                sd[b] = sd[a]
            elif b in sd and a not in sd:
                sd[a] = sd[b]
        r = super().load_state_dict(sd, strict=strict, **kw)
        self._loaded = True
        self.__dict__.pop("_oniris_lpips_pack", None)
        return r

    def _heads(self):
        return [getattr(self, f"lin{i}").model._modules["1"] for i in range(len(CHANNELS))]

    def _pack(self, device):
        """The packed weights (forward and data-gradient layouts) on `device`, rebuilt when a parameter's version changes."""
        params = list(self.parameters()) + list(self.buffers())
        sig = (str(device),) + tuple((p.data_ptr(), p._version) for p in params)
        pk = self.__dict__.get("_oniris_lpips_pack")
        if pk is not None and pk["sig"] == sig:
            return pk
        w = [c.weight.detach().to(device) for c in self._convs]
        pk = dict(sig=sig,
                  shift=self.scaling_layer.shift.detach().to(device).float().reshape(3).contiguous(),
                  scale=self.scaling_layer.scale.detach().to(device).float().reshape(3).contiguous(),
                  stem=pack_stem(w[0]), stem_bwd=pack_stem_dgrad(w[0]),
                  fwd=[None] + [pack_conv(x) for x in w[1:]], bwd=[None] + [pack_conv_dgrad(x) for x in w[1:]],
                  bias=[c.bias.detach().to(device).float().contiguous() for c in self._convs],
                  lin=[h.weight.detach().to(device).float().reshape(-1).contiguous() for h in self._heads()])
        self.__dict__["_oniris_lpips_pack"] = pk
        return pk

    def _check(self, in0, in1):
        if not self._loaded:
            raise RuntimeError("LPIPS: no weights loaded: pass weights= or call load_state_dict (the distance of an untrained net "
                               "means nothing)")
        if in0.dim() != 4 or in0.shape[1] != 3 or tuple(in0.shape) != tuple(in1.shape):
            raise ValueError(f"LPIPS: operands {tuple(in0.shape)} and {tuple(in1.shape)}: expected two equal (N, 3, H, W)")
        if in0.shape[2] < MIN_SIZE or in0.shape[3] < MIN_SIZE:
            raise ValueError(f"LPIPS: {in0.shape[2]} x {in0.shape[3]} images: H and W must be at least {MIN_SIZE}")

    def forward_torch(self, in0, in1, normalize=False):
        """The definition as plain torch code, in the operands' dtype, on any device."""
        self._check(in0, in1)
        dt = in0.dtype
        if normalize:
            in0, in1 = 2 * in0 - 1, 2 * in1 - 1
        shift, scale = self.scaling_layer.shift.to(in0.device, dt), self.scaling_layer.scale.to(in0.device, dt)
        x = torch.cat([(in0 - shift) / scale, (in1 - shift) / scale])
        N = in0.shape[0]
        total = 0
        for k, (c, h) in enumerate(zip(self._convs, self._heads())):
            if k in (1, 2):
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, c.weight.to(x.device, dt), c.bias.to(x.device, dt), stride=c.stride, padding=c.padding))
            s = x.square().sum(1, keepdim=True)
            nz = s > 0
            r = torch.where(nz, 1 / (torch.where(nz, s, torch.ones_like(s)).sqrt() + EPS), torch.zeros_like(s))
            u = x * r
            d = (u[:N] - u[N:]).square() * h.weight.to(x.device, dt)
            total = total + d.sum(1, keepdim=True).mean((2, 3), keepdim=True)
        return total

    def forward(self, in0, in1, normalize=False):
        if not (in0.is_cuda and in1.is_cuda and in0.dtype == torch.float32 and in1.dtype == torch.float32):
            return self.forward_torch(in0, in1, normalize)
        self._check(in0, in1)
        return _Distance.apply(in0, in1, self._pack(in0.device), bool(normalize))
