"""Generate ``tests/golden/ref_afnov1.npz``: recorded runs of the reference's own channels-last AFNO (networks/afnonet.py).

    MAKANI_REFERENCE=<checkout of the reference> python tests/golden/make_afnov1_golden.py

The reference's ``contractions.py``, ``activations.py``, ``layers.py`` and ``afnonet.py`` are IMPORTED from that checkout with stub
packages, the way ``make_afno_golden.py`` does.  ``makani.utils.img_utils`` (which needs ``h5py``) is a stub with a placeholder
``PeriodicPad2d``: only ``PrecipNet`` uses it.  The fixture is data only: state dicts, inputs, cotangents, outputs and gradients of

* ``net``:       a tiny ``AdaptiveFourierNeuralOperatorNet`` (24 x 40, 4 x 4 patches, 3 -> 2 channels, embed_dim 16, 2 layers,
  4 blocks, mlp_ratio 2);
* ``afno``:      ``AFNO2D(12, num_blocks=3, hard_thresholding_fraction=0.5)`` on ``[2, 8, 12, 12]`` (a window around the Nyquist row);
* ``afno_clip``: ``AFNO2D(8, num_blocks=2, hard_thresholding_fraction=1.0)`` on ``[2, 12, 6, 8]`` (the column limit, taken from
  ``H``, clipped by ``W``).

The reference's init cannot be used as it is: with scale 0.02 against a threshold of 0.01 the soft-shrink zeroes everything and
every test would pass with the filter missing.  ``w1`` / ``w2`` are drawn with std 0.4, ``b1`` / ``b2`` with std 0.3, the threshold
is 0.5; other biases and the norm weights are perturbed by 0.1.  Every ``AFNO2D`` call of the recorded runs is re-evaluated in
float64 from the hooked input, and the generator asserts that

* 20-80 % of the ReLU components and 20-80 % of the soft-shrink arguments pass, and
* no ReLU pre-activation component lies within 1e-5 rms of 0 and no soft-shrink argument within 1e-5 rms of +-lambda
  (otherwise a mask flip, not an error, would decide a gradient entry);

seeds are tried in order until all of it holds.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
STD, BIAS_STD, LAM = 0.4, 0.3, 0.5
NET_KW = dict(inp_shape=(24, 40), patch_size=(4, 4), inp_chans=3, out_chans=2, embed_dim=16, num_layers=2, num_blocks=4,
              mlp_ratio=2, sparsity_threshold=LAM)


def _load_reference():
    ref = os.environ.get("MAKANI_REFERENCE")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("set MAKANI_REFERENCE to a checkout of the reference")
    for name in ("makani", "makani.models", "makani.models.common", "makani.models.networks", "makani.utils", "makani.utils.img_utils"):
        if name not in sys.modules:
            mod = types.ModuleType(name)
            mod.__path__ = []
            sys.modules[name] = mod
    sys.modules["makani.utils.img_utils"].PeriodicPad2d = type("PeriodicPad2d", (torch.nn.Module,), {})     # PrecipNet only

    def load(modname, relpath):
        spec = importlib.util.spec_from_file_location(modname, os.path.join(ref, relpath))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[modname] = mod
        spec.loader.exec_module(mod)
        return mod

    load("makani.models.common.contractions", "makani/models/common/contractions.py")
    act = load("makani.models.common.activations", "makani/models/common/activations.py")
    lay = load("makani.models.common.layers", "makani/models/common/layers.py")
    common = sys.modules["makani.models.common"]
    common.ComplexReLU = act.ComplexReLU
    for name in ("PatchEmbed", "DropPath", "MLP"):
        setattr(common, name, getattr(lay, name))
    return load("makani.models.networks.afnonet", "makani/models/networks/afnonet.py")


def filter_margins(mod, x):
    """One ``AFNO2D`` call in float64 from its input ``[B, H, W, C]``: (ReLU pass share, soft-shrink pass share, smallest distance
    of a ReLU pre-activation component from 0, of a soft-shrink argument from +-lambda, both in units of the components' rms)."""
    B, H, W, C = x.shape
    nb, bs = mod.num_blocks, mod.block_size
    t = H // 2 + 1
    k = int(t * mod.hard_thresholding_fraction)
    c = torch.fft.rfft2(x.double(), dim=(1, 2), norm="ortho").reshape(B, H, W // 2 + 1, nb, bs)[:, t - k:t + k, :k]
    w1, b1, w2, b2 = (torch.complex(p[0].detach().double(), p[1].detach().double()) for p in (mod.w1, mod.b1, mod.w2, mod.b2))
    p1 = torch.view_as_real(torch.einsum("...ki,kio->...ko", c, w1) + b1)
    h = torch.view_as_complex(torch.relu(p1))
    p2 = torch.view_as_real(torch.einsum("...ki,kio->...ko", h, w2) + b2)
    lam = mod.sparsity_threshold
    m1 = (p1.abs().min() / p1.square().mean().sqrt()).item()
    m2 = ((p2.abs() - lam).abs().min() / p2.square().mean().sqrt()).item()
    return (p1 > 0).double().mean().item(), (p2.abs() > lam).double().mean().item(), m1, m2


def _ok(stats):
    return all(0.2 <= s[0] <= 0.8 and 0.2 <= s[1] <= 0.8 and s[2] > 1e-5 and s[3] > 1e-5 for s in stats)


def _run(mod, x, g, filters):
    """forward + backward with hooks on the filters -> (output, input gradient, margins of every filter call)."""
    seen = []
    hooks = [f.register_forward_hook(lambda m, inp, out: seen.append((m, inp[0].detach().clone()))) for f in filters]
    mod.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    y = mod(xr)
    y.backward(g)
    for h in hooks:
        h.remove()
    return y.detach(), xr.grad.detach(), [filter_margins(m, xi) for m, xi in seen]


def _record(out, prefix, mod, x, g, y, gx):
    out[f"{prefix}.x"], out[f"{prefix}.g"], out[f"{prefix}.y"], out[f"{prefix}.gx"] = x.numpy(), g.numpy(), y.numpy(), gx.numpy()
    for k, v in mod.state_dict().items():
        out[f"{prefix}.state.{k}"] = v.numpy()
    for k, p in mod.named_parameters():
        out[f"{prefix}.grad.{k}"] = p.grad.numpy()


def _seeded(build, shape_x, name):
    for seed in range(64):
        torch.manual_seed(seed)
        mod, filters = build()
        with torch.no_grad():
            for f in filters:
                for w in (f.w1, f.w2):
                    w.copy_(STD * torch.randn_like(w))
                for b in (f.b1, f.b2):
                    b.copy_(BIAS_STD * torch.randn_like(b))
            for n, p in mod.named_parameters():       # the reference's init leaves every bias 0 and every norm weight 1
                if n.endswith(".bias") or ".norm" in n:
                    p.add_(0.1 * torch.randn_like(p))
        x = torch.randn(*shape_x)
        y0 = mod(x)
        g = torch.randn_like(y0)
        y, gx, stats = _run(mod, x, g, filters)
        line = "; ".join(f"relu {s[0]:.2f} shrink {s[1]:.2f} margins {s[2]:.1e} {s[3]:.1e}" for s in stats)
        print(f"[{name}] seed {seed}: {line}", "ok" if _ok(stats) else "rejected")
        if _ok(stats):
            return seed, mod, x, g, y, gx
    raise SystemExit(f"{name}: no seed of 64 keeps the masks clear of their edges")


def main():
    afno = _load_reference()
    out = {}

    def build_net():
        net = afno.AdaptiveFourierNeuralOperatorNet(**NET_KW)
        return net, [b.filter for b in net.blocks]

    def build_filter(C, nb, frac):
        def build():
            f = afno.AFNO2D(C, num_blocks=nb, sparsity_threshold=LAM, hard_thresholding_fraction=frac)
            return f, [f]
        return build

    for name, build, shape in (("net", build_net, (2, 3, 24, 40)), ("afno", build_filter(12, 3, 0.5), (2, 8, 12, 12)),
                               ("afno_clip", build_filter(8, 2, 1.0), (2, 12, 6, 8))):
        seed, mod, x, g, y, gx = _seeded(build, shape, name)
        _record(out, name, mod, x, g, y, gx)
        out[f"{name}.seed"] = np.int64(seed)

    path = os.path.join(HERE, "ref_afnov1.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
