"""The wide VAE decoder on the GPU (csrc/vae_wide.hip, csrc/vae_wide_conv.h; autoregressive_diffusion_amd/vae.py) against the
float64 oracle (tests/vae_wide_oracle.py) and fixture G22 (the reference in float64).

Stages, through the C entry points, with operands packed by vae.py's own _pack_res_wide / _pack_lin_wide:
  exact   operands, weights and biases are seeded integers in [-3, 3]: the largest partial sum is 18 432 x 9 < 2^24, every fp32 sum
          is exact in any order, and the kernel's output must EQUAL the float64 result (torch.equal) -- every tap, channel, pixel,
          frame and batch row, no tolerance.
  float   Gaussian operands against float64, rel L2 <= 1e-5 (the project's criterion for G14 / G15 and OUT_TOL of
          tests/vae_stage_oracle.py); the activation pass element by element within 1e-5 (1 + |expected|).
Whole models: G22 (decode, chunked decode, frames, cache), a 256-wide block at g = 1 followed by a narrow one, and bit identity
of chunked / per-row decodes.  Every measured figure is printed as `vae_wide: <case> <figure>` (profiles/vae_wide_tests.txt)."""
import pytest
import torch
from torch import nn

import vae_wide_oracle as O
from test_vae_gpu import _frames_match
from test_vae_wide import g22_vae

DEV = "cuda"
pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))
TOL = 1e-5

#            C,  g, B, T,  H,  W, cache_in
CONV_CASES = [(72, 1, 2, 2, 17, 18, False),     # ragged C, one row and one column into a second tile
              (96, 2, 1, 4, 16, 33, True),      # three tile columns
              (160, 4, 1, 4, 9, 20, False),     # T = g
              (160, 4, 2, 8, 5, 7, True),
              (256, 4, 1, 8, 6, 6, True)]       # full width, two 32-channel blocks per workgroup
UP_CASES = [(96, 2, 2), (160, 1, 2), (72, 2, 1)]
_IDS = lambda c: "-".join(str(int(v)) for v in c)


def _note(case, **figs):
    print("vae_wide:", case, " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in figs.items()))


def _ints(g, *shape):
    return torch.randint(-3, 4, shape, generator=g).float()


def _lib():
    from autoregressive_diffusion_amd import _lib, vae
    return _lib, vae._stream(), vae._p


def _res_block(C, g, gen, integer):
    """A ResBlock of width C with seeded conv weights: integers in [-3, 3], or ~ N(0, 1 / fan_in) with biases ~ 0.1 N(0, 1)."""
    from autoregressive_diffusion_amd.vae import ResBlock
    rb = ResBlock(C, (2 * g, 3, 3), g, t_cond=False)
    with torch.no_grad():
        for p in (rb.conv3d0.conv3d.weight, rb.conv3d0.conv3d.bias, rb.conv3d1.weight, rb.conv3d1.bias):
            if integer:
                p.copy_(_ints(gen, *p.shape))
            else:
                p.copy_(torch.randn(p.shape, generator=gen) * (0.1 if p.dim() == 1 else p[0].numel() ** -0.5))
    return rb


def _conv_operands(case, integer):
    C, g, B, T, H, W, cached = case
    gen = torch.Generator().manual_seed(2200 + C + 7 * g + H)
    draw = (lambda *s: _ints(gen, *s)) if integer else (lambda *s: torch.randn(*s, generator=gen))
    rb = _res_block(C, g, gen, integer)
    y, res = draw(B, T, H, W, C), draw(B, T, H, W, C)
    S, _ = O.sequence(y, g, draw(B, g, H, W, C) if cached else None)
    return rb, S.contiguous(), res


def _run_convs(case, integer):
    """conv A on S and conv B on (a stand-in for u = S's last T frames, res) through the C entry points -> (a, out, a64, out64)."""
    from autoregressive_diffusion_amd.vae import _pack_res_wide
    C, g, B, T, H, W, _ = case
    L, s, p = _lib()
    rb, S, res = _conv_operands(case, integer)
    pk = _pack_res_wide(rb, C, g, dict(device=DEV, dtype=torch.float32))
    Sd, resd = S.to(DEV), res.to(DEV)
    u = Sd[:, g:].contiguous()
    a, out = torch.empty(B, T, H, W, C, device=DEV), torch.empty(B, T, H, W, C, device=DEV)
    L.check(L.lib.oniris_vae_wide_conv_a(p(Sd), p(pk["wa"]), p(pk["ba"]), p(a), B, T, H, W, C, g, s), "vae_wide_conv_a")
    L.check(L.lib.oniris_vae_wide_conv_b(p(u), p(resd), p(pk["wb"]), p(pk["bb"]), p(out), B, T, H, W, C, s), "vae_wide_conv_b")
    a64 = O.conv_a(S, rb.conv3d0.conv3d.weight.detach(), rb.conv3d0.conv3d.bias.detach(), g)
    out64 = O.conv_b(S[:, g:], res, rb.conv3d1.weight.detach(), rb.conv3d1.bias.detach())
    return a.cpu(), out.cpu(), a64, out64


@pytest.mark.parametrize("case", CONV_CASES, ids=_IDS)
def test_convs_exact(case):
    a, out, a64, out64 = _run_convs(case, integer=True)
    assert a64.abs().max() < 2 ** 24 and out64.abs().max() < 2 ** 24
    _note(f"conv exact {_IDS(case)}", a_mismatches=int((a.double() != a64).sum()), b_mismatches=int((out.double() != out64).sum()),
          a_absmax=float(a64.abs().max()))
    assert torch.equal(a, a64.float()) and torch.equal(a.double(), a64)
    assert torch.equal(out, out64.float()) and torch.equal(out.double(), out64)


@pytest.mark.parametrize("case", CONV_CASES, ids=_IDS)
def test_convs_float(case):
    a, out, a64, out64 = _run_convs(case, integer=False)
    ea, eb = O.rel_l2(a, a64), O.rel_l2(out, out64)
    _note(f"conv float {_IDS(case)}", a_rel_l2=ea, b_rel_l2=eb)
    assert ea <= TOL and eb <= TOL


@pytest.mark.parametrize("case", CONV_CASES, ids=_IDS)
def test_act_sequence_and_cache(case):
    """The activation pass in its sequence form at the conv cases' shapes: y within 1e-5 (1 + |expected|) of float64, the prefix
    EQUAL to cache_in (or to the first g frames of y), cache_out EQUAL to the last g frames of S."""
    C, g, B, T, H, W, cached = case
    L, s, p = _lib()
    gen = torch.Generator().manual_seed(2300 + C + g)
    x, emb = torch.randn(B, T, H, W, C, generator=gen) * 1.7, torch.randn(B, 2 * C, generator=gen) * 0.5
    cin = torch.randn(B, g, H, W, C, generator=gen) if cached else None
    S = torch.full((B, g + T, H, W, C), float("nan"), device=DEV)
    cout = torch.full((B, g, H, W, C), float("nan"), device=DEV)
    xd, embd, cind = x.to(DEV), emb.to(DEV), None if cin is None else cin.to(DEV)      # held: p() takes addresses only
    L.check(L.lib.oniris_vae_wide_act(p(xd), p(embd), p(cind), p(cout), p(S), B, T, H, W, C, g, s), "vae_wide_act")
    S, cout = S.cpu(), cout.cpu()
    want = O.act(x, emb)
    err = ((S[:, g:].double() - want).abs() / (1 + want.abs())).max().item()
    _note(f"act sequence {_IDS(case)}", max_scaled_err=err)
    assert err <= TOL
    assert torch.equal(S[:, :g], cin if cached else S[:, g:2 * g])
    assert torch.equal(cout, S[:, -g:])


@pytest.mark.parametrize("C", [72, 160, 256])
@pytest.mark.parametrize("with_emb", [True, False], ids=["emb", "plain"])
def test_act_plain(C, with_emb):
    """The plain form (g = 0, act2) and FiLM: every element within 1e-5 (1 + |expected|) of float64."""
    L, s, p = _lib()
    B, T, H, W = 2, 3, 5, 7
    gen = torch.Generator().manual_seed(2400 + C)
    x = torch.randn(B, T, H, W, C, generator=gen) * torch.logspace(-2, 1, T)[None, :, None, None, None]
    emb = torch.randn(B, 2 * C, generator=gen) * 0.5 if with_emb else None
    y = torch.full((B, T, H, W, C), float("nan"), device=DEV)
    xd, embd = x.to(DEV), None if emb is None else emb.to(DEV)
    L.check(L.lib.oniris_vae_wide_act(p(xd), p(embd), None, None, p(y), B, T, H, W, C, 0, s),
            "vae_wide_act")
    want = O.act(x, emb)
    err = ((y.cpu().double() - want).abs() / (1 + want.abs())).max().item()
    _note(f"act plain C={C} emb={with_emb}", max_scaled_err=err)
    assert err <= TOL


def _lin(cin, cout, gen, integer):
    m = nn.Conv3d(cin, cout, kernel_size=1)
    with torch.no_grad():
        for q in (m.weight, m.bias):
            q.copy_(_ints(gen, *q.shape) if integer else torch.randn(q.shape, generator=gen) * (0.1 if q.dim() == 1 else cin ** -0.5))
    return m


def _run_up(case, integer):
    from autoregressive_diffusion_amd.vae import _pack_lin_wide
    C, tc, sc = case
    L, s, p = _lib()
    B, T, H, W = 2, 2, 5, 18
    gen = torch.Generator().manual_seed(2500 + C)
    m = _lin(C, C * tc * sc * sc, gen, integer)
    x = _ints(gen, B, T, H, W, C) if integer else torch.randn(B, T, H, W, C, generator=gen)
    w, b = _pack_lin_wide(m.weight, m.bias, C, C, tc * sc * sc, dict(device=DEV, dtype=torch.float32))
    y = torch.full((B, T * tc, H * sc, W * sc, C), float("nan"), device=DEV)
    xd = x.to(DEV)
    L.check(L.lib.oniris_vae_wide_up(p(xd), p(w), p(b), p(y), B, T, H, W, C, tc, sc, s), "vae_wide_up")
    return y.cpu(), O.up(x, m.weight.detach(), m.bias.detach(), tc, sc)


@pytest.mark.parametrize("case", UP_CASES, ids=_IDS)
def test_up_exact(case):
    y, y64 = _run_up(case, integer=True)
    _note(f"up exact {_IDS(case)}", mismatches=int((y.double() != y64).sum()))
    assert torch.equal(y.double(), y64)


@pytest.mark.parametrize("case", UP_CASES, ids=_IDS)
def test_up_float(case):
    y, y64 = _run_up(case, integer=False)
    e = O.rel_l2(y, y64)
    _note(f"up float {_IDS(case)}", rel_l2=e)
    assert e <= TOL


def _run_out(cin, cout, integer):
    """The non-last form: all Cout channels to a contiguous channels-last buffer."""
    from autoregressive_diffusion_amd.vae import _pack_lin_wide
    L, s, p = _lib()
    B, T, H, W = 2, 2, 17, 5
    gen = torch.Generator().manual_seed(2600 + cin + cout)
    m = _lin(cin, cout, gen, integer)
    x = _ints(gen, B, T, H, W, cin) if integer else torch.randn(B, T, H, W, cin, generator=gen)
    w, b = _pack_lin_wide(m.weight, m.bias, cin, cout, 1, dict(device=DEV, dtype=torch.float32))
    y = torch.full((B, T, H, W, cout), float("nan"), device=DEV)
    xd = x.to(DEV)
    L.check(L.lib.oniris_vae_wide_out(p(xd), p(w), p(b), B, T, H, W, cin, cout, 0, None, p(y), None, *y.stride()[:4], 1, None,
                                      s), "vae_wide_out")
    return y.cpu(), O.out(x, m.weight.detach(), m.bias.detach())


@pytest.mark.parametrize("cin,cout", [(96, 48), (128, 64)])
def test_out_exact(cin, cout):
    """The area windows have length 2 here, so the mean of two integers is exact too."""
    assert all(s1 - s0 == 2 for s0, s1 in O.area_windows(cin, cout))
    y, y64 = _run_out(cin, cout, integer=True)
    _note(f"out exact {cin}-{cout}", mismatches=int((y.double() != y64).sum()))
    assert torch.equal(y.double(), y64)


@pytest.mark.parametrize("cin,cout", [(96, 48), (128, 64), (160, 72)])
def test_out_float(cin, cout):
    y, y64 = _run_out(cin, cout, integer=False)
    e = O.rel_l2(y, y64)
    _note(f"out float {cin}-{cout}", rel_l2=e)
    assert e <= TOL


def test_out_last_block_form():
    """(72, 6) with the mean | logvar split, logvar_multiplier = -1.7, strided channels-first outputs and uint8 frames."""
    from autoregressive_diffusion_amd.vae import _pack_lin_wide
    L, s, p = _lib()
    B, T, H, W, cin, cout = 2, 2, 17, 5, 72, 6
    gen = torch.Generator().manual_seed(2672)
    m = _lin(cin, cout, gen, False)
    x = torch.randn(B, T, H, W, cin, generator=gen)
    w, b = _pack_lin_wide(m.weight, m.bias, cin, cout, 1, dict(device=DEV, dtype=torch.float32))
    lvm = torch.tensor([-1.7], device=DEV)
    mean = torch.full((B, 3, T, H, W), float("nan"), device=DEV)
    logvar = torch.full_like(mean, float("nan"))
    frames = torch.zeros(B, T, H, W, 3, dtype=torch.uint8, device=DEV)
    sb, sc, st, sh, sw = mean.stride()
    xd = x.to(DEV)
    L.check(L.lib.oniris_vae_wide_out(p(xd), p(w), p(b), B, T, H, W, cin, cout, 3, p(lvm), p(mean), p(logvar), sb, st, sh, sw, sc,
                                      p(frames), s), "vae_wide_out")
    only = torch.zeros_like(frames)
    L.check(L.lib.oniris_vae_wide_out(p(xd), p(w), p(b), B, T, H, W, cin, cout, 3, p(lvm), None, None, 0, 0, 0, 0, 0, p(only), s),
            "vae_wide_out")
    m64, lv64 = O.split(O.out(x, m.weight.detach(), m.bias.detach()), -1.7)
    em, el = O.rel_l2(mean.permute(0, 2, 3, 4, 1), m64), O.rel_l2(logvar.permute(0, 2, 3, 4, 1), lv64)
    bad, off = _frames_match(frames.cpu(), torch.clip((m64 + 1) * 127.5, 0, 255))
    _note("out last block 72-6", mean_rel_l2=em, logvar_rel_l2=el, bad_pixels=bad, off_by_one=off)
    assert em <= TOL and el <= TOL and bad == 0
    assert torch.equal(only, frames)


# ---- whole models

def _g22_gpu():
    z, kw, vae = g22_vae()
    return z, kw, vae.to(DEV)


def _check_cache(vae, cache, B, h, w):
    d = vae.decoder
    assert set(cache) == {f"encoder_block_{i}" for i in range(len(d.encoder_blocks))}
    H, W = h, w
    for i, blk in enumerate(d.encoder_blocks):
        H, W = H * blk.spatial_compression, W * blk.spatial_compression
        entry = cache[f"encoder_block_{i}"]
        assert set(entry) == {f"res_block_{j}" for j in range(len(blk.res_blocks))}
        for e in entry.values():
            assert set(e) == {"conv3d_res0"}
            assert tuple(e["conv3d_res0"].shape) == (B, d.group_sizes[i], H, W, d.in_channels[i]) and e["conv3d_res0"].dtype == torch.float32


def test_decode_against_g22():
    z, kw, vae = _g22_gpu()
    zz, t = torch.from_numpy(z["z"]).to(DEV), torch.from_numpy(z["t"]).to(DEV)
    mean, logvar, cache = vae.decode(zz, t)
    em, el = O.rel_l2(mean, z["mean"]), O.rel_l2(logvar, z["logvar"])
    m0, _, c0 = vae.decode(zz[:, :, :1], t)
    m1, _, _ = vae.decode(zz[:, :, 1:], t, c0)
    ec = O.rel_l2(torch.cat((m0, m1), dim=2), z["chunked_mean"])
    frames = vae.latents_to_frames(torch.from_numpy(z["latents"]).to(DEV))
    bad, off = _frames_match(frames, z["frames_pre"])
    _note("G22 decode", mean_rel_l2=em, logvar_rel_l2=el, chunked_mean_rel_l2=ec, bad_pixels=bad, off_by_one=off)
    assert em <= TOL and el <= TOL and ec <= TOL
    assert frames.shape == z["frames_pre"].shape and bad == 0
    _check_cache(vae, cache, 2, 5, 7)
    _check_cache(vae, c0, 2, 5, 7)


def test_256_wide_then_narrow():
    """channels=[3,16,256,8], time_compressions=[1,1,2]: 256 channels at g = 1, then 16 at g = 2 -- a narrow block after a wide one."""
    from autoregressive_diffusion_amd.vae import VAE
    kw = dict(channels=[3, 16, 256, 8], n_res_blocks=1, time_compressions=[1, 1, 2], spatial_compressions=[1, 2, 2])
    vae = O.seed_params(VAE(**kw), 2256).eval()
    assert vae.decoder.in_channels == [8, 256, 16] and vae.decoder.group_sizes == [1, 1, 2]
    gen = torch.Generator().manual_seed(2257)
    zz, t = torch.randn(1, 8, 2, 3, 5, generator=gen), torch.tensor([0.2])
    m64, lv64, _ = O.decode(vae.state_dict(), kw, zz, t)
    vae = vae.to(DEV)
    mean, logvar, cache = vae.decode(zz.to(DEV), t.to(DEV))
    em, el = O.rel_l2(mean, m64), O.rel_l2(logvar, lv64)
    _note("256 wide, g = 1, then narrow", mean_rel_l2=em, logvar_rel_l2=el)
    assert em <= TOL and el <= TOL
    _check_cache(vae, cache, 1, 3, 5)


def test_chunks_and_rows_are_bit_identical():
    """On the G22 model: decoding in 1-frame chunks through the cache, and each batch row alone, gives bit for bit what the whole
    batched decode gives -- mean, logvar and the uint8 frames of decode_frames."""
    z, kw, vae = _g22_gpu()
    zz, t = torch.from_numpy(z["z"]).to(DEV), torch.from_numpy(z["t"]).to(DEV)
    lat = torch.from_numpy(z["latents"]).to(DEV)
    mean, logvar, _ = vae.decode(zz, t)
    frames, _ = vae.decode_frames(lat, 0.1)
    ms, ls, fs, cache, fcache = [], [], [], None, None
    for k in range(zz.shape[2]):
        m, l, cache = vae.decode(zz[:, :, k:k + 1], t, cache)
        f, fcache = vae.decode_frames(lat[:, k:k + 1], 0.1, fcache)
        ms.append(m); ls.append(l); fs.append(f)
    assert torch.equal(torch.cat(ms, dim=2), mean) and torch.equal(torch.cat(ls, dim=2), logvar)
    assert torch.equal(torch.cat(fs, dim=1), frames)
    for b in range(zz.shape[0]):
        m, l, _ = vae.decode(zz[b:b + 1], t[b:b + 1])
        f, _ = vae.decode_frames(lat[b:b + 1], 0.1)
        assert torch.equal(m, mean[b:b + 1]) and torch.equal(l, logvar[b:b + 1]) and torch.equal(f, frames[b:b + 1])
    _note("bit identity", chunks=zz.shape[2], rows=zz.shape[0])
