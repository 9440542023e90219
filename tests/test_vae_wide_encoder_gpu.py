"""The wide VAE encoder on the GPU (oniris_vae_wide_down of csrc/vae_wide.hip / csrc/vae_wide_conv.h, the wide ResBlock launches with a
null FiLM pointer; autoregressive_diffusion_amd/vae.py) against the float64 oracle (tests/vae_wide_encoder_oracle.py) and fixture
G23 (the reference in float64).

  down exact   operands, weights and biases are seeded integers in [-3, 3] and every area window has a power-of-two length: every fp32
               sum is exact in any order (|partial sums| <= 1024 x 9 < 2^24, the mean has at most 7 fractional bits), and the kernel's
               output must EQUAL the float64 result.
  down float   Gaussian operands against float64, rel L2 <= 1e-5 (the project's criterion for G14 / G15 and tests/test_vae_wide_gpu.py).
Whole models: G23 (encode, chunked encode, encode_long_sequence, latents, cache), the reference's shape [3,16,64,256,8], bit identity
of chunked / per-row / uint8 / strided encodes, and forward in eval mode.  Every measured figure is printed as
`vae_wide_enc: <case> <figure>` (profiles/vae_wide_encoder_tests.txt)."""
import functools

import pytest
import torch
from torch import nn

import vae_wide_oracle as O
import vae_wide_encoder_oracle as E
from test_vae_wide_encoder import CS_KW, g23_vae

DEV = "cuda"
pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))
TOL = 1e-5

B, TO, HO, WO = 2, 2, 17, 18                     # one row and one column of output pixels in a second tile
#              Cin, tc, sc, Cout
EXACT_CASES = [(3, 1, 1, 72),                    # windows of length 1, odd Cin, ragged CP
               (72, 1, 2, 144),                  # length 2, scalar staging
               (64, 2, 2, 256),                  # length 2, vector staging, NB = 2, all 8 sub-positions
               (256, 1, 2, 8)]                   # length 128, narrow output
FLOAT_CASES = EXACT_CASES + [(72, 2, 2, 160),    # K = 576, ragged windows
                             (96, 2, 2, 100)]    # a window crosses a sub-position boundary
_IDS = lambda c: "-".join(str(int(v)) for v in c)


def _note(case, **figs):
    print("vae_wide_enc:", case, " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in figs.items()))


def _lib():
    from autoregressive_diffusion_amd import _lib, vae
    return _lib, vae._stream(), vae._p


def _down_operands(case, integer):
    Cin, tc, sc, Cout = case
    K = Cin * tc * sc * sc
    gen = torch.Generator().manual_seed(2320 + Cin + 3 * Cout + tc)
    m = nn.Conv3d(K, Cout, kernel_size=1)
    with torch.no_grad():
        for q in (m.weight, m.bias):
            q.copy_(torch.randint(-3, 4, q.shape, generator=gen).float() if integer
                    else torch.randn(q.shape, generator=gen) * (0.1 if q.dim() == 1 else K ** -0.5))
    shape = (B, TO * tc, HO * sc, WO * sc, Cin)
    x = torch.randint(-3, 4, shape, generator=gen).float() if integer else torch.randn(shape, generator=gen)
    return m, x


def _launch_down(case, m, xd, strides, normalize):
    """oniris_vae_wide_down on the device tensor xd addressed by `strides` (b, t, h, w, c) into a NaN-filled buffer."""
    from autoregressive_diffusion_amd.vae import _pack_down_wide
    Cin, tc, sc, Cout = case
    L, s, p = _lib()
    w, b = _pack_down_wide(m.weight, m.bias, Cin, Cout, tc * sc * sc, dict(device=DEV, dtype=torch.float32))
    y = torch.full((B, TO, HO, WO, Cout), float("nan"), device=DEV)
    L.check(L.lib.oniris_vae_wide_down(p(xd), int(xd.dtype == torch.uint8), *strides, B, TO, HO, WO, Cin, tc, sc, int(normalize), p(w),
                                       p(b), Cout, p(y), s), "vae_wide_down")
    return y.cpu()


def _cl_strides(xd):
    return xd.stride()[:4] + (1,)


@pytest.mark.parametrize("case", EXACT_CASES, ids=_IDS)
def test_down_exact(case):
    Cin, tc, sc, Cout = case
    lens = {s1 - s0 for s0, s1 in O.area_windows(Cin * tc * sc * sc, Cout)}
    assert all(n & (n - 1) == 0 for n in lens) and lens == {{3: 1, 72: 2, 64: 2, 256: 128}[Cin]}
    m, x = _down_operands(case, integer=True)
    want = E.down(x, m.weight.detach(), m.bias.detach(), tc, sc)
    assert want.abs().max() < 2 ** 16
    y = _launch_down(case, m, x.to(DEV), _cl_strides(x), False)
    _note(f"down exact {_IDS(case)}", mismatches=int((y.double() != want).sum()), absmax=float(want.abs().max()))
    assert torch.equal(y.double(), want)
    if Cin != 3:
        return
    # the same from a uint8 tensor (operands 0 .. 6, normalize = 0) and from a strided (B, C, T, H, W) fp32 view
    u8 = (x + 3).to(torch.uint8)
    want8 = E.down(u8.double(), m.weight.detach(), m.bias.detach(), tc, sc)
    y8 = _launch_down(case, m, u8.to(DEV), _cl_strides(u8), False)
    xs = x.permute(0, 4, 1, 2, 3).contiguous().to(DEV)
    sb, scs, st, sh, sw = xs.stride()
    ys = _launch_down(case, m, xs, (sb, st, sh, sw, scs), False)
    _note(f"down exact {_IDS(case)} forms", u8_mismatches=int((y8.double() != want8).sum()), strided_mismatches=int((ys != y).sum()))
    assert torch.equal(y8.double(), want8) and torch.equal(ys, y)


@pytest.mark.parametrize("case", FLOAT_CASES, ids=_IDS)
def test_down_float(case):
    Cin, tc, sc, Cout = case
    if case == (96, 2, 2, 100):
        assert any(s0 // Cin != (s1 - 1) // Cin for s0, s1 in O.area_windows(Cin * tc * sc * sc, Cout))
    m, x = _down_operands(case, integer=False)
    want = E.down(x, m.weight.detach(), m.bias.detach(), tc, sc)
    y = _launch_down(case, m, x.to(DEV), _cl_strides(x), False)
    e = O.rel_l2(y, want)
    _note(f"down float {_IDS(case)}", rel_l2=e, nans=int(y.isnan().sum()))
    assert not y.isnan().any() and e <= TOL


@pytest.mark.parametrize("case", [(3, 1, 1, 72), (96, 2, 2, 100)], ids=_IDS)
def test_down_uint8_normalized(case):
    Cin, tc, sc, Cout = case
    m, _ = _down_operands(case, integer=False)
    gen = torch.Generator().manual_seed(2330 + Cin)
    u8 = torch.randint(0, 256, (B, TO * tc, HO * sc, WO * sc, Cin), generator=gen, dtype=torch.uint8)
    want = E.down(u8.double() / 127.5 - 1, m.weight.detach(), m.bias.detach(), tc, sc)
    y = _launch_down(case, m, u8.to(DEV), _cl_strides(u8), True)
    e = O.rel_l2(y, want)
    _note(f"down uint8 normalize {_IDS(case)}", rel_l2=e, nans=int(y.isnan().sum()))
    assert not y.isnan().any() and e <= TOL


#                                     C, g, B, T, H, W, cache_in
@pytest.mark.parametrize("case", [(160, 2, 2, 4, 5, 7, True), (72, 4, 1, 8, 9, 6, False)], ids=_IDS)
def test_act_sequence_null_emb(case):
    """The activation pass in its sequence form as the encoder calls it (emb NULL): y within 1e-5 (1 + |expected|) of float64, the
    prefix EQUAL to cache_in (or to the first g frames of y), cache_out EQUAL to the last g frames of S."""
    C, g, Bn, T, H, W, cached = case
    L, s, p = _lib()
    gen = torch.Generator().manual_seed(2340 + C + g)
    x = torch.randn(Bn, T, H, W, C, generator=gen) * 1.7
    cin = torch.randn(Bn, g, H, W, C, generator=gen) if cached else None
    S = torch.full((Bn, g + T, H, W, C), float("nan"), device=DEV)
    cout = torch.full((Bn, g, H, W, C), float("nan"), device=DEV)
    xd, cind = x.to(DEV), None if cin is None else cin.to(DEV)                  # held: p() takes addresses only
    L.check(L.lib.oniris_vae_wide_act(p(xd), None, p(cind), p(cout), p(S), Bn, T, H, W, C, g, s), "vae_wide_act")
    S, cout = S.cpu(), cout.cpu()
    want = O.act(x)
    err = ((S[:, g:].double() - want).abs() / (1 + want.abs())).max().item()
    _note(f"act sequence, null emb {_IDS(case)}", max_scaled_err=err)
    assert err <= TOL
    assert torch.equal(S[:, :g], cin if cached else S[:, g:2 * g])
    assert torch.equal(cout, S[:, -g:])


# ---- whole models

@functools.lru_cache(maxsize=None)
def _g23_gpu():
    z, kw, vae = g23_vae()
    return z, kw, vae.to(DEV)


def _check_cache(vae, cache, Bn, H, W):
    enc = vae.encoder
    assert set(cache) == {f"encoder_block_{i}" for i in range(len(enc.encoder_blocks))}
    for i, blk in enumerate(enc.encoder_blocks):
        H, W = H // blk.spatial_compression, W // blk.spatial_compression
        entry = cache[f"encoder_block_{i}"]
        assert set(entry) == {f"res_block_{j}" for j in range(len(blk.res_blocks))}
        for e in entry.values():
            assert set(e) == {"conv3d_res0"}
            assert tuple(e["conv3d_res0"].shape) == (Bn, enc.group_sizes[i], H, W, enc.out_channels[i])
            assert e["conv3d_res0"].dtype == torch.float32


def test_encode_against_g23():
    z, kw, vae = _g23_gpu()
    x = torch.from_numpy(z["x"]).float().to(DEV)
    mean, cache = vae.encode(x)
    m0, c0 = vae.encode(x[:, :, :4])
    m1, _ = vae.encode(x[:, :, 4:], c0)
    long = vae.encode_long_sequence(x.cpu(), split_size=4)
    em, ec = O.rel_l2(mean, z["mean"]), O.rel_l2(torch.cat((m0, m1), dim=2), z["chunked_mean"])
    el = O.rel_l2(long, z["mean"])
    _note("G23 encode", mean_rel_l2=em, chunked_mean_rel_l2=ec, long_sequence_rel_l2=el)
    assert mean.shape == z["mean"].shape and em <= TOL and ec <= TOL and el <= TOL
    _check_cache(vae, cache, 2, 20, 28)
    _check_cache(vae, c0, 2, 20, 28)
    with pytest.raises(ValueError, match="cache"):
        vae.encode(x[:1, :, 4:], c0)


def test_frames_to_latents_against_g23():
    z, kw, vae = _g23_gpu()
    frames = torch.from_numpy(z["frames"]).to(DEV)
    lat, cache = vae.encode_frames(frames)
    lat2 = vae.frames_to_latents(frames)
    e = O.rel_l2(lat, z["latents"])
    _note("G23 frames_to_latents", latents_rel_l2=e)
    assert lat.shape == z["latents"].shape and e <= TOL and torch.equal(lat, lat2)
    _check_cache(vae, cache, 2, 20, 28)


def test_reference_shape():
    """channels=[3,16,64,256,8]: narrow, narrow, wide (K = 512), a wide `down` (K = 1024) into narrow ResBlocks.  8 frames: the
    shortest sequence this model takes, in the reference too -- the encoder's group sizes are [4, 4, 2, 1], and block 1 (g = 4)
    sees T / 2 frames, which must fill one group."""
    from autoregressive_diffusion_amd.vae import VAE
    vae = O.seed_params(VAE(**CS_KW), 2356).eval()
    gen = torch.Generator().manual_seed(2357)
    x = torch.rand(1, 3, 8, 16, 16, generator=gen) * 2 - 1
    want, _ = E.encode(vae.state_dict(), CS_KW, x)
    vae = vae.to(DEV)
    routes = [(bool(bk.get("wide")), bool(bk.get("wide_down"))) for bk in vae._pack_encoder(torch.device(DEV, 0))["blocks"]]
    assert routes == [(False, False), (False, False), (True, True), (False, True)]
    mean, cache = vae.encode(x.to(DEV))
    e = O.rel_l2(mean, want)
    _note("reference shape [3,16,64,256,8]", mean_rel_l2=e)
    assert mean.shape == (1, 8, 2, 2, 2) and e <= TOL
    with pytest.raises(ValueError, match="multiple of 8"):
        vae.encode(x[:, :, :4].to(DEV))
    _check_cache(vae, cache, 1, 16, 16)


def test_encodes_are_bit_identical():
    """On the G23 model: chunks (4, 4) through the cache, each batch row alone, uint8 frames against the same frames as float32 and a
    strided input against its contiguous copy give bit for bit what the whole batched encode gives."""
    z, kw, vae = _g23_gpu()
    x = torch.from_numpy(z["x"]).float().to(DEV)
    frames = torch.from_numpy(z["frames"]).to(DEV)
    mean, _ = vae.encode(x)
    lat, _ = vae.encode_frames(frames)
    m0, c = vae.encode(x[:, :, :4])
    m1, _ = vae.encode(x[:, :, 4:], c)
    l0, c = vae.encode_frames(frames[:, :4])
    l1, _ = vae.encode_frames(frames[:, 4:], c)
    assert torch.equal(torch.cat((m0, m1), dim=2), mean) and torch.equal(torch.cat((l0, l1), dim=1), lat)
    for b in range(x.shape[0]):
        assert torch.equal(vae.encode(x[b:b + 1])[0], mean[b:b + 1])
        assert torch.equal(vae.encode_frames(frames[b:b + 1])[0], lat[b:b + 1])
    assert torch.equal(vae.encode_frames(frames.float())[0], lat)
    xs = x.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)             # channels-last memory behind (B, 3, T, H, W)
    fs = frames.permute(0, 4, 1, 2, 3).contiguous().permute(0, 2, 3, 4, 1)        # channels-first memory behind (B, T, H, W, 3)
    assert not xs.is_contiguous() and not fs.is_contiguous()
    assert torch.equal(vae.encode(xs)[0], vae.encode(xs.contiguous())[0]) and torch.equal(vae.encode(xs)[0], mean)
    assert torch.equal(vae.encode_frames(fs)[0], vae.encode_frames(fs.contiguous())[0]) and torch.equal(vae.encode_frames(fs)[0], lat)
    _note("bit identity", chunks=2, rows=x.shape[0])


def test_forward_eval_and_training_refusal():
    """forward in eval mode with t_sample and noise given: mean is encode's, (r_mean, r_logvar) are decode's of the mix, bit for bit;
    the training path still refuses, naming the width."""
    from autoregressive_diffusion_amd.edm2.utils import bmult
    z, kw, vae = _g23_gpu()
    x = torch.from_numpy(z["x"]).float().to(DEV)
    gen = torch.Generator().manual_seed(2370)
    t_b = (torch.rand(2, generator=gen) * 0.3).to(DEV)
    noise = torch.randn(z["mean"].shape, generator=gen).to(DEV)
    try:
        r_mean, r_logvar, mean, cache = vae.eval()(x, t_sample=t_b, noise=noise)
        want_mean, _ = vae.encode(x)
        mix = bmult(want_mean, 1 - t_b) + bmult(noise, t_b)
        want_r, want_lv, _ = vae.decode(mix, t_b)
        assert torch.equal(mean, want_mean) and torch.equal(r_mean, want_r) and torch.equal(r_logvar, want_lv)
        assert set(cache) == {"encoder", "decoder"} and r_mean.grad_fn is None
        _check_cache(vae, cache["encoder"], 2, 20, 28)
        with pytest.raises(NotImplementedError, match=r"160 channels.*edm2\.vae"):
            vae.train()(x)
    finally:
        vae.eval()
    _note("forward eval", r_mean_absmax=float(r_mean.abs().max()))
