"""Bit identity of the VAE's host layer between two trees (profiles/host_layer_one_block.txt, step 2): the sibling of
scratch/disc_shared_parts_bits.py for `vae.py` / `vae_train.py`.

  python scratch/vae_host_layer_bits.py run DIR        in a tree, in a fresh process: every case below on seeded inputs; every output,
                                                       cache entry and parameter gradient goes to DIR/tensors.pt
  python scratch/vae_host_layer_bits.py compare A B    torch.equal on every tensor of the two runs, no tolerance; one line per case

Cases (scratch/launch_trace.py records the launches of the same ones): encode, decode, decode_frames and encode_frames of a narrow
VAE, each in two chunks through the cache; one training forward + backward of a small narrow VAE (channels [3, 8, 8], 8 frames of
16 x 16); one decode of a wide VAE (widths up to 128), in two chunks through the cache.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scratch")]
import torch  # noqa: E402

DEV = "cuda"
NARROW = dict(channels=[3, 8, 16, 8], n_res_blocks=2, mean=[0.1 * i for i in range(8)], std=[1.0 + 0.1 * i for i in range(8)])
TRAIN = dict(channels=[3, 8, 8], n_res_blocks=1, time_compressions=[2, 2], spatial_compressions=[2, 2])
WIDE = dict(channels=[3, 16, 128, 8], n_res_blocks=1, time_compressions=[1, 2, 1], spatial_compressions=[1, 2, 2],
            mean=[0.0] * 8, std=[1.0] * 8)


def model(kw, seed):
    from autoregressive_diffusion_amd.vae import VAE
    from vae_wide_oracle import seed_params
    torch.manual_seed(seed)
    return seed_params(VAE(**kw), seed).to(DEV)


def flat(cache, prefix):
    """The tensors of a nested cache dict under joined keys."""
    if isinstance(cache, dict):
        out = {}
        for k, v in cache.items():
            out.update(flat(v, f"{prefix}/{k}"))
        return out
    return {} if cache is None else {prefix: cache}


def chunked(fn, x, dim, names):
    """fn(chunk, cache) -> (*outputs, cache) over the two halves of x along dim: the second call reads the first one's cache."""
    t, cache = {}, None
    for i, c in enumerate(x.chunk(2, dim)):
        *outs, cache = fn(c, cache)
        t.update({f"{n}{i}": o for n, o in zip(names, outs)})
        t.update(flat(cache, f"cache{i}"))
    return t


def training(vae):
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(2, 3, 8, 16, 16, generator=g) * 2 - 1).to(DEV)
    ts, noise = (torch.rand(2, generator=g) * 0.1).to(DEV), torch.randn(2, 8, 2, 4, 4, generator=g).to(DEV)
    r_mean, r_logvar, mean, _ = vae(x, t_sample=ts, noise=noise)
    (0.5 * (r_logvar + (x - r_mean) ** 2 / torch.exp(r_logvar)).mean() + 0.1 * mean.square().mean()).backward()
    t = dict(r_mean=r_mean, r_logvar=r_logvar, mean=mean)
    for n, p in vae.named_parameters():
        assert p.grad is not None, n
        t["grad/" + n] = p.grad
    return t


def cases():
    g = torch.Generator().manual_seed(9)
    narrow, wide, train = model(NARROW, 31).eval(), model(WIDE, 32).eval(), model(TRAIN, 33).train()
    x = (torch.rand(2, 3, 8, 32, 32, generator=g) * 2 - 1).to(DEV)
    frames = torch.randint(0, 256, (2, 8, 32, 32, 3), generator=g, dtype=torch.uint8).to(DEV)
    z, lat = torch.randn(2, 8, 4, 8, 8, generator=g).to(DEV), torch.randn(2, 4, 8, 8, 8, generator=g).to(DEV)
    zw = torch.randn(1, 8, 4, 6, 5, generator=g).to(DEV)
    tt = torch.tensor([0.05, 0.1]).to(DEV)
    return {
        "vae_encode": lambda: chunked(lambda c, k: narrow.encode(c, k), x, 2, ["mean"]),
        "vae_decode": lambda: chunked(lambda c, k: narrow.decode(c, tt, k), z, 2, ["mean", "logvar"]),
        "vae_decode_frames": lambda: chunked(lambda c, k: narrow.decode_frames(c, 0.1, k), lat, 1, ["frames"]),
        "vae_encode_frames": lambda: chunked(lambda c, k: narrow.encode_frames(c, k), frames, 1, ["latents"]),
        "vae_train": lambda: training(train),
        "vae_wide_decode": lambda: chunked(lambda c, k: wide.decode(c, 0.1, k), zw, 2, ["mean", "logvar"]),
    }


def run(outdir):
    os.makedirs(outdir, exist_ok=True)
    out = {}
    for name, fn in cases().items():
        t = fn()
        torch.cuda.synchronize()
        for k, v in t.items():
            out[f"{name}//{k}"] = v.detach().cpu().clone()
        print(name, len(t), "tensors", flush=True)
    torch.save(out, os.path.join(outdir, "tensors.pt"))
    print(f"saved {len(out)} tensors, {sum(v.numel() for v in out.values())} elements")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        from disc_shared_parts_bits import compare
        sys.exit(compare(sys.argv[2], sys.argv[3]))
