"""Generate tests/golden/ref_stepper.npz: inputs, cached state and outputs of the reference's own
``makani/models/preprocessor.py`` and ``makani/models/stepper.py``.

Run in the build container (the reference tree is mounted read-only there):

    python tests/golden/make_stepper_golden.py

The two modules are imported by file path (package ``__init__`` files bypassed, as in make_golden.py) with stubs for
what they import and this machine lacks: ``makani.utils.comm`` (every size 1), ``makani.utils.grids.GridConverter``
(hands back the coordinates it is given), ``modulus.distributed.mappings`` (identities) and
``makani.utils.conditioning_inputs`` (hands back the arrays stored in the path attributes).  With those the reference
runs the cases below; the fork's wrappers hard-code a mask on channel 20 of sample 0, ``MultiStepWrapper.forward``
raises (its ``_forward_train`` / ``_forward_eval`` are called directly) and ``history_denormalize`` raises in the
statistics modes, so the wrappers run in mode "none".

The fixture is data only (inputs, toy-model weights, expected outputs); no reference source text is stored.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


class Params:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def base_params(H, W, **kw):
    p = dict(n_history=0, history_normalization_mode="none", history_normalization_decay=0.5, target="default",
             normalize_residual=False, img_shape_x=H, img_shape_y=W, img_local_offset_x=0, img_local_offset_y=0,
             img_local_shape_x=H, img_local_shape_y=W, add_grid=False, gridtype="sinusoidal", grid_num_frequencies=2,
             data_grid_type="equiangular", model_grid_type="equiangular", add_orography=False, add_landmask=False,
             n_future=0)
    p.update(kw)
    return Params(**p)


def _load_reference_modules():
    def stub(name, **attrs):
        mod = types.ModuleType(name)
        mod.__path__ = []
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
        return mod

    class GridConverter:
        def __init__(self, src, dst, lat, lon):
            assert src == dst
            self.lat, self.lon = lat, lon

        def get_dst_coords(self):
            return self.lat, self.lon

    for name in ("makani", "makani.models", "makani.utils", "modulus", "modulus.distributed"):
        stub(name)
    stub("makani.utils.comm", get_size=lambda name: 1, get_rank=lambda name: 0)
    sys.modules["makani.utils"].comm = sys.modules["makani.utils.comm"]
    stub("makani.utils.grids", GridConverter=GridConverter)
    stub("modulus.distributed.mappings", reduce_from_parallel_region=lambda x, name: x, copy_to_parallel_region=lambda x, name: x)
    stub("makani.utils.conditioning_inputs", get_orography=lambda a: a, get_land_mask=lambda a: a)

    def load(modname, relpath):
        spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, relpath))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[modname] = mod
        spec.loader.exec_module(mod)
        return mod

    pre = load("makani.models.preprocessor", "makani/models/preprocessor.py")
    stp = load("makani.models.stepper", "makani/models/stepper.py")
    return pre, stp


def toy_model(cin, cout, g):
    m = torch.nn.Conv2d(cin, cout, 1)
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=g) / cin ** 0.5)
        m.bias.copy_(torch.randn(m.bias.shape, generator=g))
    return m


def main():
    pre, stp = _load_reference_modules()
    g = torch.Generator().manual_seed(2024)
    out = {}

    def randn(*shape):
        return torch.randn(*shape, generator=g)

    # ---- single: SingleStepWrapper at B = 1, 22 predicted + 1 unpredicted channel, sinusoidal grid from lat / lon,
    # orography and land mask; the fork masks channel 20 of input and output with the last static channel
    H, W, C, Cu = 4, 6, 22, 1
    lat = np.linspace(90.0, -90.0, H).astype(np.float32)
    lon = np.linspace(0.0, 360.0, W, endpoint=False).astype(np.float32)
    oro = torch.rand(H, W, generator=g).numpy()
    oro = ((oro - oro.min()) / (oro.max() - oro.min())).astype(np.float32)        # what the loader hands over: [0, 1]
    lsm = (torch.rand(H, W, generator=g) > 0.5).numpy().astype(np.int64)
    p = base_params(H, W, add_grid=True, lat=lat, lon=lon, add_orography=True, orography_path=oro, add_landmask=True,
                    landmask_path=lsm)
    Cs = 4 + 1 + 2
    model = toy_model(C + Cu + Cs, C, g)
    wrap = stp.SingleStepWrapper(p, lambda: model)
    wrap.eval()
    inp, xz = randn(1, C, H, W), randn(1, 1, Cu, H, W)
    wrap.preprocessor.cache_unpredicted_features(None, None, xz, None)
    with torch.no_grad():
        y = wrap(inp)
    out.update(single_lat=lat, single_lon=lon, single_oro=oro, single_lsm=lsm, single_w=model.weight.detach().numpy(),
               single_b=model.bias.detach().numpy(), single_inp=inp.numpy(), single_xz=xz.numpy(), single_y=y.numpy(),
               single_static=wrap.preprocessor.static_features.numpy())

    # ---- multi: MultiStepWrapper._forward_train (with input gradient) and _forward_eval, mode "none", n_future = 1,
    # unpredicted input and target channels, sinusoidal grid features of the default linspace grid
    H, W, B, C, Cu, Cs = 4, 6, 2, 3, 1, 4
    for nh in (0, 1):
        T = nh + 1
        p = base_params(H, W, n_history=nh, n_future=1, add_grid=True)
        model = toy_model(T * (C + Cu) + Cs, C, g)
        wrap = stp.MultiStepWrapper(p, lambda: model)
        k = f"multi{nh}_"
        inp, xz, yz, cot = randn(B, T * C, H, W), randn(B, T, Cu, H, W), randn(B, 2, Cu, H, W), randn(B, 2 * C, H, W)
        out.update({k + "w": model.weight.detach().numpy(), k + "b": model.bias.detach().numpy(), k + "inp": inp.numpy(),
                    k + "xz": xz.numpy(), k + "yz": yz.numpy(), k + "cot": cot.numpy()})
        wrap.train()
        wrap.preprocessor.cache_unpredicted_features(None, None, xz.clone(), yz.clone())
        # the state cache_unpredicted_features sets is xz / yz themselves (recorded above); what append_history makes of
        # it during the rollout is recorded below
        assert torch.equal(wrap.preprocessor.unpredicted_inp_train, xz) and torch.equal(wrap.preprocessor.unpredicted_tar_train, yz)
        x = inp.clone().requires_grad_(True)
        res = wrap._forward_train(x)
        (res * cot).sum().backward()
        out.update({k + "train_y": res.detach().numpy(), k + "train_ginp": x.grad.numpy(),
                    k + "train_uinp_after": wrap.preprocessor.unpredicted_inp_train.numpy().copy()})
        wrap.eval()
        wrap.preprocessor.cache_unpredicted_features(None, None, xz.clone(), yz.clone())
        with torch.no_grad():
            out[k + "eval_y"] = wrap._forward_eval(inp).numpy()
        if nh == 1:
            # ---- the small methods, on this preprocessor (evaluation mode, freshly cached unpredicted channels)
            pp = wrap.preprocessor
            x1, x2, xc = randn(B, T * C, H, W), randn(B, C, H, W), randn(B, T * Cu, H, W)
            with torch.no_grad():
                out["meth_x1"], out["meth_x2"], out["meth_xc"] = x1.numpy(), x2.numpy(), xc.numpy()
                out["meth_append_channels"] = pp.append_channels(x1, xc).numpy()
                assert torch.equal(pp.flatten_history(pp.append_channels(pp.expand_history(x1, T), xc)), pp.append_channels(x1, xc))
                out["meth_add_static"] = pp.add_static_features(x1).numpy()
                # the remove_* methods and flatten(expand(.)) hand back their input: checked here, nothing to store
                assert torch.equal(pp.remove_static_features(pp.add_static_features(x1)), x1)
                xa = pp.append_unpredicted_features(x1)
                out["meth_append_unpredicted"] = xa.numpy()
                assert torch.equal(pp.remove_unpredicted_features(xa), x1)
                out["meth_append_history"] = pp.append_history(x1, x2, 1).numpy()
                out["meth_uinp_after_append_history"] = pp.unpredicted_inp_eval.numpy().copy()
                assert torch.equal(pp.flatten_history(pp.expand_history(x1, T)), x1)

    # ---- residual: add_residual at n_history = 0 with normalize_residual, input without gradient
    H, W, B, C = 5, 8, 2, 3
    scale = (0.5 + torch.rand(1, C, 1, 1, generator=g)).numpy().astype(np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "time_diff_stds.npy")
        np.save(path, scale)
        pp = pre.Preprocessor2D(base_params(H, W, target="residual", normalize_residual=True, time_diff_stds_path=path))
    x, dx = randn(B, C, H, W), randn(B, C, H, W)
    out.update(resid_scale=scale, resid_x=x.numpy().copy(), resid_dx=dx.numpy())
    with torch.no_grad():
        out["resid_y"] = pp.add_residual(x.clone(), dx).numpy()

    # ---- stats: history_compute_stats + history_normalize of input and target, mode "exponential"
    H, W, B, C, Cu, nh = 4, 6, 2, 3, 1, 2
    pp = pre.Preprocessor2D(base_params(H, W, n_history=nh, history_normalization_mode="exponential"))
    chan_scale = 0.3 + 2.7 * torch.rand(1, 1, C + Cu, 1, 1, generator=g)
    chan_off = 2.0 * chan_scale * (2 * torch.rand(1, 1, C + Cu, 1, 1, generator=g) - 1)
    xa = randn(B, nh + 1, C + Cu, H, W) * chan_scale + chan_off
    tar = randn(B, C, H, W) * chan_scale[:, 0, :C] + chan_off[:, 0, :C]
    with torch.no_grad():
        pp.history_compute_stats(xa)
        out.update(stats_xa=xa.numpy(), stats_tar=tar.numpy(),
                   stats_weights=pp.history_normalization_weights.numpy(), stats_mean=pp.history_mean.numpy(),
                   stats_std=pp.history_std.numpy(), stats_xn=pp.history_normalize(pp.flatten_history(xa), target=False).numpy(),
                   stats_tarn=pp.history_normalize(tar, target=True).numpy())

    path = os.path.join(HERE, "ref_stepper.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
