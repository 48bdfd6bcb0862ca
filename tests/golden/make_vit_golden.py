"""Generate ``tests/golden/ref_vit.npz``: a recorded run of the reference's own ViT (networks/vit.py).

    MAKANI_REFERENCE=<checkout of the reference> python tests/golden/make_vit_golden.py

The reference's ``layers.py`` and ``vit.py`` are IMPORTED from that checkout with stub packages, the way ``make_afno_golden.py``
does; ``vit.py`` also needs ``makani.utils.comm`` (a stub whose ``get_size`` returns 1) and the three distributed names of
``makani.mpu.layers`` (stubs that are never constructed).  The fixture is data only: state dict, input, cotangent, output,
input gradient and parameter gradients of

    VisionTransformer(inp_shape=[21, 40], patch_size=(7, 8), inp_chans=3, out_chans=2, embed_dim=64, depth=2, num_heads=2,
                      mlp_ratio=1.0)   at batch 2:  3 x 5 = 15 tokens, head size 32.

The reference's init cannot be used as it is: with std 0.02 every score is about 0, the softmax is a mean, and a kernel without
the exponential would pass.  ``qkv.weight`` is drawn with std ``QKV_STD``, every bias and norm weight gets ``0.1 randn`` added,
and for every attention call of the recorded run the scaled scores are re-evaluated in float64 from the hooked input: the
generator asserts that their standard deviation lies between 1 and 3.  Seeds are tried in order until that holds.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
QKV_STD = 0.2
NET_KW = dict(inp_shape=[21, 40], patch_size=(7, 8), inp_chans=3, out_chans=2, embed_dim=64, depth=2, num_heads=2, mlp_ratio=1.0)
BATCH = 2


def _load_reference():
    ref = os.environ.get("MAKANI_REFERENCE")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("set MAKANI_REFERENCE to a checkout of the reference")
    for name in ("makani", "makani.models", "makani.models.common", "makani.models.networks", "makani.utils", "makani.mpu"):
        if name not in sys.modules:
            mod = types.ModuleType(name)
            mod.__path__ = []
            sys.modules[name] = mod
    comm = types.ModuleType("makani.utils.comm")
    comm.get_size = lambda name: 1
    sys.modules["makani.utils.comm"] = sys.modules["makani.utils"].comm = comm
    mpu = types.ModuleType("makani.mpu.layers")
    for name in ("DistributedMatmul", "DistributedMLP", "DistributedAttention"):
        setattr(mpu, name, type(name, (), {}))
    sys.modules["makani.mpu.layers"] = mpu

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
    return load("makani.models.networks.vit", "makani/models/networks/vit.py")


def score_std(attn, x):
    """Standard deviation of the scaled scores of one attention call, in float64 from its input."""
    B, N, C = x.shape
    H, D = attn.num_heads, attn.head_dim
    w, b = attn.qkv.weight.detach().double(), attn.qkv.bias
    qkv = x.double() @ w.t() + (b.detach().double() if b is not None else 0.0)
    q, k, _ = qkv.reshape(B, N, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
    return float((q @ k.transpose(-1, -2) * attn.scale).std())


def main():
    vit = _load_reference()
    for seed in range(64):
        torch.manual_seed(seed)
        net = vit.VisionTransformer(**NET_KW)
        with torch.no_grad():
            for n, p in net.named_parameters():
                if n.endswith("qkv.weight"):
                    p.copy_(QKV_STD * torch.randn_like(p))
                if n.endswith(".bias") or ".norm" in n or n.startswith("norm."):
                    p.add_(0.1 * torch.randn_like(p))
        x = torch.randn(BATCH, NET_KW["inp_chans"], *NET_KW["inp_shape"])
        seen = []
        hooks = [b.attn.register_forward_hook(lambda m, inp, out: seen.append(score_std(m, inp[0].detach()))) for b in net.blocks]
        xr = x.clone().requires_grad_(True)
        y = net(xr)
        g = torch.randn_like(y)
        y.backward(g)
        for h in hooks:
            h.remove()
        ok = len(seen) == len(net.blocks) and all(1.0 < s < 3.0 for s in seen)
        print(f"seed {seed}: score std {', '.join(f'{s:.2f}' for s in seen)}", "ok" if ok else "rejected")
        if ok:
            break
    else:
        raise SystemExit("no seed of 64 gives scores with a standard deviation between 1 and 3")
    out = {"x": x.numpy(), "g": g.numpy(), "y": y.detach().numpy(), "gx": xr.grad.numpy(), "seed": np.int64(seed),
           "score_std": np.array(seen)}
    for k, v in net.state_dict().items():
        out[f"state.{k}"] = v.numpy()
    for k, p in net.named_parameters():
        out[f"grad.{k}"] = p.grad.numpy()
    path = os.path.join(HERE, "ref_vit.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
