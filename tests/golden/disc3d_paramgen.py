"""The nets of fixture G20 (Discriminator3D alone; make_golden_disc3d.py).  Parameters and inputs come from disc_paramgen:
fill(disc3d_shapes(in_channels, widths), seed) loaded strict=True, inputs(shape, seed); the cotangent is cot(., 0.3).

Between them the four nets hold T = 1, odd and even extents under stride 2, stem outputs wider than one 16-pixel tile (c3: 18, d3:
17), GroupNorm groups of 1, 2 and 3 channels, both shortcut forms, unequal last widths and N = 1."""

# name -> (in_channels, widths, input (N, C, T, H, W), seed)
G20_NETS = {"a3": (3, (32,), (2, 3, 1, 7, 5), 2001), "b3": (6, (32, 64), (2, 6, 5, 18, 22), 2002),
            "c3": (3, (96, 32, 32), (1, 3, 9, 20, 36), 2003), "d3": (8, (64, 96), (3, 8, 2, 33, 17), 2004)}
G20_LOGITS = {"a3": (2, 2, 1, 4, 3), "b3": (2, 2, 2, 5, 6), "c3": (1, 2, 2, 3, 5), "d3": (3, 2, 1, 9, 5)}
# conv1 with 32 output channels feeds a GroupNorm whose groups are single channels: these bias gradients are mathematically zero
G20_ZERO_BIAS = {"a3": ("blocks.0.conv1.bias",), "b3": ("blocks.0.conv1.bias",), "c3": ("blocks.1.conv1.bias", "blocks.2.conv1.bias"),
                 "d3": ()}
G20_FULL_MAX = 16384          # gradients of at most this many elements are stored in full
PHI = 0.3


def grad_entries(key, g):
    """What G20 stores of the gradient g (a torch tensor) of parameter `key`: {entry name: tensor}.  Small gradients in full; of the
    larger ones (all of them 27-tap weights) the norm, the 27 per-tap Frobenius norms and output channels 0..3 in full."""
    if g.numel() <= G20_FULL_MAX:
        return {"grad/" + key: g}
    assert g.dim() == 5 and tuple(g.shape[2:]) == (3, 3, 3), key
    return {"gradnorm/" + key: g.norm(), "gradtaps/" + key: g.pow(2).sum((0, 1)).sqrt().reshape(27), "gradhead/" + key: g[:4]}
