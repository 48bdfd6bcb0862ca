"""Generate ``tests/golden/ref_afno.npz``: recorded runs of the reference's own AFNO (networks/afnonet_v2.py).

    MAKANI_REFERENCE=<checkout of the reference> python tests/golden/make_afno_golden.py

The reference's ``contractions.py``, ``activations.py``, ``layers.py`` and ``afnonet_v2.py`` are IMPORTED from that checkout with
stub packages (``makani/__init__.py`` pulls in the trainer and its absent dependencies), the way ``make_golden.py`` does.  The
fixture is data only: state dicts, inputs, cotangents, outputs and gradients of

* ``net``:  a tiny ``AdaptiveFourierNeuralOperatorNet`` (24 x 40, 4 x 4 patches, 3 -> 2 channels, embed_dim 16, 2 layers, 4 blocks,
  mlp_ratio 2, instance norm, linear skip);
* ``afno``: one ``AFNO2D`` alone with ``hard_thresholding_fraction=0.5`` (the two-slice branch);
* ``pe``:   one ``PatchEmbed``.

The reference's init cannot be used as it is: with scale 0.02 against a threshold of 0.01 the soft-shrink zeroes every
coefficient (the filter's own output has rms 4e-9) and every test would pass with the filter missing.  ``w1`` / ``w2`` are
drawn with std 0.4 and the threshold is 0.5 (with std 0.25 the soft-shrink arguments of these shapes have rms 0.26 and only
3-11 % of them pass, whatever the seed; the second product's rms grows with the square of the std).  For every ``AFNO2D`` call of the recorded runs the call is re-evaluated in
float64 from the hooked input, and the generator asserts that

* 20-80 % of the ReLU components and 20-80 % of the soft-shrink arguments pass, and
* no ReLU pre-activation component lies within 1e-5 rms of 0 and no soft-shrink argument within 1e-5 rms of +-lambda
  (otherwise a mask flip, not an error, would decide a gradient entry);

seeds are tried in order until both hold.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
STD, LAM = 0.4, 0.5
NET_KW = dict(inp_shape=(24, 40), patch_size=(4, 4), inp_chans=3, out_chans=2, embed_dim=16, num_layers=2, num_blocks=4,
              mlp_ratio=2, normalization_layer="instance_norm", skip_fno="linear", sparsity_threshold=LAM)


def _load_reference():
    ref = os.environ.get("MAKANI_REFERENCE")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("set MAKANI_REFERENCE to a checkout of the reference")
    for name in ("makani", "makani.models", "makani.models.common", "makani.models.networks"):
        if name not in sys.modules:
            mod = types.ModuleType(name)
            mod.__path__ = []
            sys.modules[name] = mod

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
    return load("makani.models.networks.afnonet_v2", "makani/models/networks/afnonet_v2.py"), lay


def filter_margins(mod, x):
    """One ``AFNO2D`` call in float64 from its input: (ReLU pass share, soft-shrink pass share, smallest distance of a ReLU
    pre-activation component from 0, of a soft-shrink argument from +-lambda, both in units of the components' rms)."""
    B, C, H, W = x.shape
    nb, bs = mod.num_blocks, mod.block_size
    th, tw = H // 2 + 1, W // 2 + 1
    kh, kw = int(th * mod.hard_thresholding_fraction), int(tw * mod.hard_thresholding_fraction)
    c = torch.fft.rfft2(x.double(), dim=(-2, -1), norm="ortho").view(B, nb, bs, H, tw)[..., :kw]
    if kh != th:
        c = torch.cat([c[:, :, :, :kh], c[:, :, :, -kh:]], dim=3)
    w1, w2 = (torch.view_as_complex(w.detach().double().contiguous()) for w in (mod.w1, mod.w2))
    p1 = torch.view_as_real(torch.einsum("bkixy,kio->bkoxy", c, w1))
    h = torch.view_as_complex(torch.relu(p1))
    p2 = torch.view_as_real(torch.einsum("bkixy,kio->bkoxy", h, w2))
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
                f.w1.copy_(STD * torch.randn_like(f.w1))
                f.w2.copy_(STD * torch.randn_like(f.w2))
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
    afno, lay = _load_reference()
    out = {}

    def build_net():
        net = afno.AdaptiveFourierNeuralOperatorNet(**NET_KW)
        return net, [b.filter for b in net.blocks]

    seed, net, x, g, y, gx = _seeded(build_net, (2, 3, 24, 40), "net")
    _record(out, "net", net, x, g, y, gx)
    out["net.seed"] = np.int64(seed)

    def build_filter():
        f = afno.AFNO2D(12, num_blocks=3, sparsity_threshold=LAM, hard_thresholding_fraction=0.5)
        return f, [f]

    seed, f, x, g, y, gx = _seeded(build_filter, (2, 12, 8, 12), "afno")
    _record(out, "afno", f, x, g, y, gx)
    out["afno.seed"] = np.int64(seed)

    torch.manual_seed(0)
    pe = lay.PatchEmbed(img_size=(8, 12), patch_size=(2, 3), in_chans=3, embed_dim=5)
    x = torch.randn(2, 3, 8, 12)
    g = torch.randn(2, 5, 16)
    y, gx, _ = _run(pe, x, g, [])
    _record(out, "pe", pe, x, g, y, gx)

    path = os.path.join(HERE, "ref_afno.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
