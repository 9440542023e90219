"""The C-ABI calls of the discriminator and the VAE, call by call, for comparing two trees (profiles/host_layer_one_block.txt,
step 1): a refactor of the Python layer must leave them equal line for line.

  python scratch/launch_trace.py run FILE         in a tree, in a fresh process: every case below; one line per call goes to FILE
  python scratch/launch_trace.py compare A B      the two files line by line; prints the first differing lines, exit status 1 if any

`_lib.lib` is replaced by a forwarding proxy (the mechanism of ONIRIS_HOST_TIMING=2 in _lib.py).  Per call the line holds the case,
the entry point and every argument by `_lib._SIGS`: integers and floats by value, ctypes arrays by content, pointers as NULL or PTR
(addresses are not comparable across trees).

Cases: the whole nets of scratch/disc_shared_parts_bits.py (net2d_train, net2d_eval, net3d, mixed_discriminator_loss,
mixed_vae_loss) and the VAE cases of scratch/vae_host_layer_bits.py.
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scratch")]


def show(a, ctype):
    if isinstance(a, ctypes.Array):
        return "[" + " ".join(map(repr, a)) + "]"
    if ctype in (ctypes.c_void_p, ctypes.c_char_p) or not isinstance(a, (int, float)):
        if isinstance(a, ctypes.c_void_p):
            a = a.value
        return "NULL" if a is None or a == 0 else "PTR"
    return repr(float(a)) if ctype in (ctypes.c_float, ctypes.c_double) else repr(int(a))


class Proxy:
    """Forwards every attribute to the loaded library; calls of the entry points in _SIGS are written down first."""

    def __init__(self, lib, sigs, lines):
        self._lib, self.case = lib, "-"
        for name, (_, argtypes) in sigs.items():
            setattr(self, name, self._recorded(name, getattr(lib, name), argtypes, lines))

    def _recorded(self, name, fn, argtypes, lines):
        def call(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            lines.append(f"{self.case} | {name}(" + ", ".join(show(a, t) for a, t in zip(args, argtypes)) + ")")
            return fn(*args)
        return call

    def __getattr__(self, name):
        return getattr(self._lib, name)


def run(path):
    import torch
    from autoregressive_diffusion_amd import _lib, discriminator as d
    import disc_shared_parts_bits as disc_cases
    import vae_host_layer_bits as vae_cases
    lines = []
    cases = dict(disc_cases.nets(d))                     # built, like the VAE models, before the proxy goes in
    cases.update(vae_cases.cases())
    _lib.lib = proxy = Proxy(_lib.lib, _lib._SIGS, lines)
    for name, fn in cases.items():
        proxy.case, before = name, len(lines)
        fn()
        torch.cuda.synchronize()
        print(name, len(lines) - before, "calls", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {len(lines)} calls of {len({ln.split(' | ')[1].split('(')[0] for ln in lines})} entry points")


def compare(pa, pb):
    a, b = open(pa).read().splitlines(), open(pb).read().splitlines()
    differ = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    per = {}
    for ln in a:
        per[ln.split(" | ")[0]] = per.get(ln.split(" | ")[0], 0) + 1
    for case, n in per.items():
        print(f"{case}: {n} calls")
    print(f"{len(a)} and {len(b)} lines: {len(differ)} differ" + ("" if len(a) == len(b) else "; the lengths differ"))
    for i in differ[:10]:
        print(f"line {i + 1}:\n  {a[i]}\n  {b[i]}")
    return 0 if not differ and len(a) == len(b) else 1


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
