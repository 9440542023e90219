"""Gradients of the native discriminators do not depend on which other gradients were asked for: the `needs_input_grad` bookkeeping
of the two autograd Functions of autoregressive_diffusion_amd/discriminator.py (the conv stage and the Block, shared by the 2-D and
the 3-D half).

Per net one reference run with everything trainable and the input requiring grad, then runs from fresh nets (same state dict, same
input, same cotangent) with only a subset trainable.  Each gradient comes from the same launch on the same operands whichever of
its neighbours is requested, and every sum has a fixed order, so the comparison is torch.equal, no tolerance.

Nets: Discriminator2D(3, (32, 32)) on (2, 3, 9, 7) -- ragged tiles, one downsampling block and one block with the identity
shortcut -- and Discriminator3D(3, (32, 64)) on (2, 3, 3, 9, 7) -- one downsampling block, one final block with the 1x1x1 shortcut
conv, and both rules for conv1's bias gradient (32 output channels: exactly zero, nothing launched; 64: computed).  No GroupNorm
there sees a single value: the smallest group holds 6.  The last subset is the one case in which a Block's input needs no
gradient while its first norm does (want_dx = False), which no whole net with a trainable stem reaches."""
import pytest
import torch

import disc_paramgen as G

DEV = "cuda"
pytestmark = pytest.mark.gpu

NETS = {"2d": ("Discriminator2D", G.disc2d_shapes, (32, 32), (2, 3, 9, 7), 2301),
        "3d": ("Discriminator3D", G.disc3d_shapes, (32, 64), (2, 3, 3, 9, 7), 2302)}
# name -> (which parameters train, whether the input requires grad)
SUBSETS = {"norms": (lambda k: "norm" in k, True),
           "conv_biases": (lambda k: k.endswith(("conv1.bias", "conv2.bias")), True),
           "shortcuts": (lambda k: ".shortcut." in k, True),
           "no_dx": (lambda k: k.startswith("blocks.0.norm1.") or k == "blocks.1.conv1.weight", False)}
_reference = {}


def run(net_name, trainable, want_dx):
    """Train-mode logits and gradients of a fresh net in which the parameters chosen by `trainable` require grad."""
    from autoregressive_diffusion_amd import discriminator as d
    cls, shapes, widths, shape, seed = NETS[net_name]
    net = getattr(d, cls)(3, widths)
    net.load_state_dict(G.fill(shapes(3, widths), seed), strict=True)
    net = net.to(DEV).train()
    for k, p in net.named_parameters():
        p.requires_grad_(bool(trainable(k)))
    x = G.inputs(shape, seed).to(DEV).requires_grad_(want_dx)
    logits = net(x)
    (logits * G.cot(logits.shape, 0.3, torch.float32).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return logits.detach(), x.grad, {k: p.grad for k, p in net.named_parameters()}


def reference(net_name):
    if net_name not in _reference:
        _reference[net_name] = run(net_name, lambda k: True, True)
    return _reference[net_name]


@pytest.mark.parametrize("subset", list(SUBSETS))
@pytest.mark.parametrize("net_name", list(NETS))
def test_gradients_do_not_depend_on_what_else_is_requested(net_name, subset):
    trainable, want_dx = SUBSETS[subset]
    ref_logits, ref_dx, ref_grads = reference(net_name)
    logits, dx, grads = run(net_name, trainable, want_dx)
    assert torch.equal(logits, ref_logits)
    if want_dx:
        assert dx is not None and torch.equal(dx, ref_dx)
    else:
        assert dx is None
    chosen = [k for k in grads if trainable(k)]
    assert chosen and set(grads) == set(ref_grads)
    for k, g in grads.items():
        if k not in chosen:
            assert g is None, k
        elif "conv_norm_out" in k:                       # unused, as in the reference: no gradient in any run
            assert g is None and ref_grads[k] is None, k
        else:
            assert g is not None and tuple(g.shape) == tuple(ref_grads[k].shape) and torch.equal(g, ref_grads[k]), k
    produced = [k for k in chosen if grads[k] is not None]
    print(f"{net_name} {subset}: {len(produced)} gradients equal to the reference run's, {len(grads) - len(chosen)} frozen "
          f"parameters without one, dx {'equal' if want_dx else 'not requested'}")
    assert produced
