"""CPU tests of Preprocessor2D and the step wrappers against the reference's recorded results
(tests/golden/ref_stepper.npz, written by tests/golden/make_stepper_golden.py from the reference's own modules) and
against float64 restatements written here.

Mode "none" is concatenation, tiling, a mask and the toy model -- the same torch ops as the reference's -- so every
recorded output and the input gradient must match bit for bit.  The history statistics are formed from raw float64 sums
here and from fp32 reductions in the reference: mean and std agree within 1e-6 (the mean relative to the std; the
project's raw-sum tolerance, test_metrics_gpu.py) and normalised fields within 2e-6 relative L2 (the project's field
tolerance, test_lploss_gpu.py).  The reference's own fp32 path measured against float64 stays within 2.8e-7 and 7.7e-7
(absolute, |x| <= 7.5) on such fields, inside both bounds.  Test inputs keep |mean| <= 3 std so that the one-pass
variance loses nothing visible in float64."""
import os

import numpy as np
import pytest
import torch

import capi_checks as capi

from makani_amd.preprocessor import Preprocessor2D, get_preprocessor
from makani_amd.stepper import MultiStepWrapper, SingleStepWrapper

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_stepper.npz")
STAT_TOL = 1e-6
FIELD_TOL = 2e-6


class Params:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def make_params(H, W, **kw):
    p = dict(n_history=0, history_normalization_mode="none", history_normalization_decay=0.5, target="default",
             normalize_residual=False, img_shape_x=H, img_shape_y=W, img_local_offset_x=0, img_local_offset_y=0,
             img_local_shape_x=H, img_local_shape_y=W, add_grid=False, gridtype="sinusoidal", grid_num_frequencies=2,
             data_grid_type="equiangular", model_grid_type="equiangular", add_orography=False, add_landmask=False,
             n_future=0)
    p.update(kw)
    return Params(**p)


def gold():
    return {k: torch.from_numpy(v) for k, v in np.load(GOLD).items()}


def toy_model(w, b):
    m = torch.nn.Conv2d(w.shape[1], w.shape[0], 1)
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    return m


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return (torch.linalg.norm(a - b) / torch.linalg.norm(b)).item()


def scaled_fields(shape, seed, lo=0.3, hi=3.0, off=2.0):
    """``[B, T, Cn, H, W]`` fp32 fields with a per-channel scale in [lo, hi] and an offset of up to ``off`` sigma."""
    g = torch.Generator().manual_seed(seed)
    cn = shape[2]
    scale = lo + (hi - lo) * torch.rand(1, 1, cn, 1, 1, generator=g)
    offset = off * scale * (2 * torch.rand(1, 1, cn, 1, 1, generator=g) - 1)
    return torch.randn(*shape, generator=g) * scale + offset


def stats_f64(xa, weights, n):
    """The reference's definition in float64: m = sum_t w_t sum_hw x / N, var = sum_t w_t sum_hw (x - m)^2 / N."""
    w = weights.double().reshape(1, -1, 1, 1, 1)
    x = xa.double()
    m = (x * w).sum((1, 3, 4), keepdim=True) / n
    var = ((x - m) ** 2 * w).sum((1, 3, 4), keepdim=True) / n
    return m.squeeze(1), var.sqrt().squeeze(1)           # [B, Cn, 1, 1]


def check_stats(pp, xa, n, what=""):
    m64, s64 = stats_f64(xa, pp.history_normalization_weights, n)
    em = ((pp.history_mean.double() - m64).abs() / s64).max().item()
    es = ((pp.history_std.double() - s64).abs() / s64).max().item()
    print(f"{what} mean err / std {em:.2e}, std rel err {es:.2e} (bound {STAT_TOL:.0e})")
    assert pp.history_mean.dtype == torch.float32 and pp.history_std.dtype == torch.float32
    assert em < STAT_TOL and es < STAT_TOL
    return m64, s64


# ---------------------------------------------------------------------------- mode "none": bit for bit
def test_single_step_wrapper_equals_the_fork_bit_for_bit(tmp_path):
    g = gold()
    H, W = g["single_oro"].shape
    np.save(tmp_path / "oro.npy", g["single_oro"].numpy())
    np.save(tmp_path / "lsm.npy", g["single_lsm"].numpy())
    p = make_params(H, W, add_grid=True, lat=g["single_lat"].numpy(), lon=g["single_lon"].numpy(), add_orography=True,
                    orography_path=str(tmp_path / "oro.npy"), add_landmask=True, landmask_path=str(tmp_path / "lsm.npy"),
                    masked_channels=[20])
    wrap = SingleStepWrapper(p, lambda: toy_model(g["single_w"], g["single_b"]))
    wrap.eval()
    assert torch.equal(wrap.preprocessor.static_features, g["single_static"])
    wrap.preprocessor.cache_unpredicted_features(None, None, g["single_xz"].clone(), None)
    with torch.no_grad():
        y = wrap(g["single_inp"])
    assert torch.equal(y, g["single_y"])
    # without the mask list the wrapper is upstream's: channel 20 differs, and only because of the mask
    p.masked_channels = []
    plain = SingleStepWrapper(p, lambda: toy_model(g["single_w"], g["single_b"]))
    plain.eval()
    plain.preprocessor.cache_unpredicted_features(None, None, g["single_xz"].clone(), None)
    with torch.no_grad():
        y0 = plain(g["single_inp"])
    assert not torch.equal(y0, y)


@pytest.mark.parametrize("nh", [0, 1])
def test_multi_step_wrapper_equals_the_reference_bit_for_bit(nh):
    g = gold()
    k = f"multi{nh}_"
    H, W = g[k + "inp"].shape[-2:]
    p = make_params(H, W, n_history=nh, n_future=1, add_grid=True)
    wrap = MultiStepWrapper(p, lambda: toy_model(g[k + "w"], g[k + "b"]))
    wrap.train()
    wrap.preprocessor.cache_unpredicted_features(None, None, g[k + "xz"].clone(), g[k + "yz"].clone())
    x = g[k + "inp"].clone().requires_grad_(True)
    y = wrap(x)
    (y * g[k + "cot"]).sum().backward()
    assert torch.equal(y.detach(), g[k + "train_y"])
    assert torch.equal(x.grad, g[k + "train_ginp"])
    assert torch.equal(wrap.preprocessor.unpredicted_inp_train, g[k + "train_uinp_after"])
    wrap.eval()
    wrap.preprocessor.cache_unpredicted_features(None, None, g[k + "xz"].clone(), g[k + "yz"].clone())
    with torch.no_grad():
        assert torch.equal(wrap(g[k + "inp"]), g[k + "eval_y"])


def test_small_methods_equal_the_reference_bit_for_bit():
    g = gold()
    H, W = g["meth_x1"].shape[-2:]
    pp = get_preprocessor(make_params(H, W, n_history=1, n_future=1, add_grid=True))
    assert isinstance(pp, Preprocessor2D)
    pp.eval()
    pp.cache_unpredicted_features(None, None, g["multi1_xz"].clone(), g["multi1_yz"].clone())
    x1, x2, xc = g["meth_x1"], g["meth_x2"], g["meth_xc"]
    assert torch.equal(pp.append_channels(x1, xc), g["meth_append_channels"])
    assert pp.append_channels(pp.expand_history(x1, 2), xc).dim() == 5
    assert torch.equal(pp.flatten_history(pp.append_channels(pp.expand_history(x1, 2), xc)), g["meth_append_channels"])
    xs = pp.add_static_features(x1)
    assert torch.equal(xs, g["meth_add_static"])
    assert torch.equal(pp.remove_static_features(xs), x1)
    xa = pp.append_unpredicted_features(x1)
    assert torch.equal(xa, g["meth_append_unpredicted"])
    assert torch.equal(pp.remove_unpredicted_features(xa), x1)
    assert torch.equal(pp.append_history(x1, x2, 1), g["meth_append_history"])
    assert torch.equal(pp.unpredicted_inp_eval, g["meth_uinp_after_append_history"])
    assert torch.equal(pp.flatten_history(pp.expand_history(x1, 2)), x1)
    # the assembly of mode "none" is those methods composed
    assert torch.equal(pp.assemble(x1), pp.add_static_features(pp.append_unpredicted_features(x1)))


def test_add_residual(tmp_path):
    g = gold()
    H, W = g["resid_x"].shape[-2:]
    np.save(tmp_path / "tds.npy", g["resid_scale"].numpy())
    pp = Preprocessor2D(make_params(H, W, target="residual", normalize_residual=True, time_diff_stds_path=str(tmp_path / "tds.npy")))
    x = g["resid_x"].clone()
    y = pp.add_residual(x, g["resid_dx"])
    assert torch.equal(y, g["resid_y"])
    assert torch.equal(x, g["resid_x"])                  # out of place, unlike the reference
    # with a history it returns the new last step, which append_history takes
    pp1 = Preprocessor2D(make_params(H, W, n_history=1, target="residual", normalize_residual=True,
                                     time_diff_stds_path=str(tmp_path / "tds.npy")))
    xh = torch.cat([torch.zeros_like(x), x], dim=1)
    y1 = pp1.add_residual(xh, g["resid_dx"])
    assert torch.equal(y1, g["resid_y"])
    assert pp1.append_history(xh, y1, 0).shape == xh.shape
    # direct learning: the prediction itself
    assert Preprocessor2D(make_params(H, W)).add_residual(x, g["resid_dx"]) is g["resid_dx"]


# ---------------------------------------------------------------------------- statistics modes
def test_statistics_against_the_reference_and_float64():
    g = gold()
    xa, tar = g["stats_xa"], g["stats_tar"]
    B, T, Cn, H, W = xa.shape
    pp = Preprocessor2D(make_params(H, W, n_history=T - 1, history_normalization_mode="exponential"))
    assert torch.equal(pp.history_normalization_weights, g["stats_weights"])
    pp.history_compute_stats(xa)
    m64, s64 = check_stats(pp, xa, H * W, "golden")
    assert pp.history_mean.shape == g["stats_mean"].shape and pp.history_std.shape == g["stats_std"].shape
    # the reference's recorded fp32 values
    assert ((pp.history_mean - g["stats_mean"]).abs() / g["stats_std"]).max() < STAT_TOL
    assert ((pp.history_std - g["stats_std"]).abs() / g["stats_std"]).max() < STAT_TOL
    xn = pp.history_normalize(pp.flatten_history(xa), target=False)
    tn = pp.history_normalize(tar, target=True)
    xn64 = ((xa.double() - m64.unsqueeze(1)) / s64.unsqueeze(1)).reshape(B, T * Cn, H, W)
    tn64 = (tar.double() - m64[:, :tar.shape[1]]) / s64[:, :tar.shape[1]]
    for got, want in ((xn, xn64), (xn, g["stats_xn"]), (tn, tn64), (tn, g["stats_tarn"])):
        assert got.shape == want.shape and got.dtype == torch.float32
        print(f"normalised field rel L2 {rel(got, want):.2e} (bound {FIELD_TOL:.0e})")
        assert rel(got, want) < FIELD_TOL
    assert pp.history_normalize(xa, target=False).shape == xa.shape                # 5-D in, 5-D out


@pytest.mark.parametrize("H,W", [(9, 16), (33, 60), (91, 180)])
@pytest.mark.parametrize("mode", ["exponential", "mean"])
def test_assemble_statistics_and_round_trip(H, W, mode):
    B, T, C, Cu = 2, 3, 4, 1
    xa = scaled_fields((B, T, C + Cu, H, W), seed=H + (mode == "mean"))
    x, u = xa[:, :, :C].contiguous(), xa[:, :, C:].contiguous()
    pp = Preprocessor2D(make_params(H, W, n_history=T - 1, history_normalization_mode=mode, add_grid=True))
    pp.eval()
    pp.cache_unpredicted_features(None, None, u, None)
    out = pp.assemble(pp.flatten_history(x))
    m64, s64 = check_stats(pp, xa, H * W, f"{mode} {H}x{W}")
    Cd = T * (C + Cu)
    assert out.shape == (B, Cd + 4, H, W) and out.dtype == torch.float32
    want = ((xa.double() - m64.unsqueeze(1)) / s64.unsqueeze(1)).reshape(B, Cd, H, W)
    print(f"assembled field rel L2 {rel(out[:, :Cd], want):.2e}")
    assert rel(out[:, :Cd], want) < FIELD_TOL
    assert torch.equal(out[:, Cd:], pp.static_features.expand(B, -1, -1, -1))
    # denormalising the normalised target gives the target back
    tar = xa[:, -1, :C].contiguous()
    back = pp.history_denormalize(pp.history_normalize(tar, target=True), target=True)
    assert rel(back, tar) < FIELD_TOL
    full = pp.flatten_history(xa)
    assert rel(pp.history_denormalize(pp.history_normalize(full, target=False), target=False), full) < FIELD_TOL


def test_gradient_through_the_statistics_is_autograd():
    H, W, B, T, C = 9, 16, 2, 2, 3
    xa = scaled_fields((B, T, C, H, W), seed=5)
    pp = Preprocessor2D(make_params(H, W, n_history=T - 1, history_normalization_mode="exponential"))
    x = pp.flatten_history(xa).clone().requires_grad_(True)
    cot = torch.randn(B, T * C, H, W, generator=torch.Generator().manual_seed(6))
    (pp.assemble(x) * cot).sum().backward()
    x64 = xa.double().clone().requires_grad_(True)
    w = pp.history_normalization_weights.double()
    m = (x64 * w).sum((1, 3, 4), keepdim=True) / (H * W)
    s = (((x64 - m) ** 2 * w).sum((1, 3, 4), keepdim=True) / (H * W)).sqrt()
    (((x64 - m) / s).reshape(B, T * C, H, W) * cot.double()).sum().backward()
    assert rel(x.grad, x64.grad.reshape(B, T * C, H, W)) < 1e-5


# ---------------------------------------------------------------------------- the documented deviations
def test_modes_mean_and_timediff():
    pp = Preprocessor2D(make_params(4, 6, n_history=3, history_normalization_mode="mean"))
    assert torch.equal(pp.history_normalization_weights, torch.full((1, 4, 1, 1, 1), 0.25))
    with pytest.raises(NotImplementedError):
        Preprocessor2D(make_params(4, 6, n_history=1, history_normalization_mode="timediff"))
    assert "history_normalization_weights" not in pp.state_dict() and not pp.state_dict()


def test_static_inputs_from_npy_and_missing_readers(tmp_path):
    H, W = 6, 8
    g = torch.Generator().manual_seed(3)
    raw = (1000.0 * torch.rand(H, W, generator=g)).numpy()
    lsm = (torch.rand(1, H, W, generator=g) > 0.4).numpy().astype(np.int64)      # [1, H, W] as the reference's file holds it
    np.save(tmp_path / "oro.npy", raw)
    np.save(tmp_path / "lsm.npy", lsm)
    p = make_params(H, W, add_grid=True, gridtype="linear", add_orography=True, orography_path=str(tmp_path / "oro.npy"),
                    add_landmask=True, landmask_path=str(tmp_path / "lsm.npy"), img_local_offset_x=2, img_local_shape_x=3,
                    img_local_offset_y=4, img_local_shape_y=4)
    pp = Preprocessor2D(p)
    sf = pp.static_features
    assert sf.shape == (1, 2 + 1 + 2, 3, 4)
    tx = torch.linspace(0, 1, H + 1)[:-1]
    ty = torch.linspace(0, 1, W + 1)[:-1]
    assert torch.equal(sf[0, 0], tx[2:5, None].expand(3, 4)) and torch.equal(sf[0, 1], ty[None, 4:8].expand(3, 4))
    o = torch.tensor((raw - raw.min()) / (raw.max() - raw.min()), dtype=torch.float32)
    o = (o - o.mean()) / (o.std() + 1.0e-6)
    assert torch.equal(sf[0, 2], o[2:5, 4:8])
    m = torch.from_numpy(lsm[0])[2:5, 4:8]
    assert torch.equal(sf[0, 3], (m == 0).float()) and torch.equal(sf[0, 4], (m == 1).float())
    # sinusoidal: (sin x, sin y) per frequency
    p.gridtype, p.grid_num_frequencies = "sinusoidal", 3
    sf = Preprocessor2D(p).static_features
    assert sf.shape[1] == 6 + 3
    gx = tx[2:5, None].expand(3, 4)
    assert torch.equal(sf[0, 0], torch.sin(gx)) and torch.equal(sf[0, 4], torch.sin(3 * gx))
    # other formats need the reference's reader libraries
    for lib, key in (("netCDF4", "orography_path"), ("h5py", "landmask_path")):
        try:
            __import__(lib)
        except ImportError:
            setattr(p, key, str(tmp_path / "file.nc"))
            with pytest.raises(ImportError, match=lib):
                Preprocessor2D(p)
            setattr(p, key, str(tmp_path / ("oro.npy" if key == "orography_path" else "lsm.npy")))
    # differing grids would need the GridConverter interpolation
    q = make_params(H, W, add_grid=True, lat=np.linspace(90, -90, H), lon=np.linspace(0, 360, W, endpoint=False),
                    model_grid_type="legendre-gauss")
    with pytest.raises(NotImplementedError):
        Preprocessor2D(q)


def test_masked_channels():
    H, W, B, T, C, Cu = 5, 8, 2, 2, 3, 1
    g = torch.Generator().manual_seed(9)
    x, u = torch.randn(B, T * C, H, W, generator=g), torch.randn(B, T, Cu, H, W, generator=g)
    plain = Preprocessor2D(make_params(H, W, n_history=T - 1, add_grid=True))
    masked = Preprocessor2D(make_params(H, W, n_history=T - 1, add_grid=True, masked_channels=[1]))
    for pp in (plain, masked):
        pp.eval()
        pp.cache_unpredicted_features(None, None, u.clone(), None)
    a, b = plain.assemble(x), masked.assemble(x)
    mask = plain.static_features[:, -1]
    hit = [1, (C + Cu) + 1]                                # channel 1 of both history steps, all samples
    for c in range(a.shape[1]):
        assert torch.equal(b[:, c], a[:, c] * mask if c in hit else a[:, c]), c
    y = torch.randn(B, C, H, W, generator=g)
    ym = masked.mask_output(y)
    assert torch.equal(ym[:, 1], y[:, 1] * mask) and torch.equal(ym[:, [0, 2]], y[:, [0, 2]])
    assert plain.mask_output(y) is y
    with pytest.raises(ValueError):
        Preprocessor2D(make_params(H, W, masked_channels=[0]))            # no static feature to mask with
    bad = Preprocessor2D(make_params(H, W, add_grid=True, masked_channels=[7]))
    with pytest.raises(ValueError):
        bad.assemble(torch.randn(B, C, H, W))


def test_assemble_returns_its_argument_when_nothing_is_to_do():
    pp = Preprocessor2D(make_params(4, 6))
    x = torch.randn(2, 3, 4, 6)
    assert pp.assemble(x) is x and pp.assemble(x, out_dtype=torch.float32) is x
    assert pp.assemble(x, out_dtype=torch.bfloat16).dtype == torch.bfloat16


def test_state_dict_keys_are_the_models():
    from makani_amd.sfnonet import SphericalFourierNeuralOperatorNet
    H, W = 17, 32
    kw = dict(inp_shape=(H, W), out_shape=(H, W), scale_factor=2, inp_chans=3 + 4, out_chans=3, embed_dim=6, num_layers=2)
    keys = ["model." + k for k in SphericalFourierNeuralOperatorNet(**kw).state_dict()]
    assert keys
    for cls in (SingleStepWrapper, MultiStepWrapper):
        wrap = cls(make_params(H, W, add_grid=True, n_future=1), lambda: SphericalFourierNeuralOperatorNet(**kw))
        assert list(wrap.state_dict()) == keys
        assert isinstance(wrap.preprocessor, Preprocessor2D) and isinstance(wrap.model, SphericalFourierNeuralOperatorNet)


# ---------------------------------------------------------------------------------------------------------------------
# misaligned pointers: refused by the host checks, with the message of the check (tests/capi_checks.py)
# ---------------------------------------------------------------------------------------------------------------------
_A = capi.A
MISALIGNED = [      # entry point, its arguments in front of the stream with one pointer moved off its alignment, the refusal
    ("mk_input_assemble", (_A + 2, 0, None, None, None, None, None, 0, 0, _A, 0, 1, 2, 3, 0, 0, 4, 8), "x or output not aligned to its element"),
    ("mk_input_assemble", (_A, 1, None, None, None, None, None, 0, 0, _A + 1, 1, 1, 2, 3, 0, 0, 4, 8), "x or output not aligned to its element"),
    ("mk_input_assemble", (_A, 0, _A, _A, _A + 2, _A, None, 0, 0, _A, 0, 1, 2, 3, 1, 1, 4, 8), "fp32 / int32 stream not 4-byte aligned"),
    ("mk_input_assemble", (_A, 0, None, _A, None, None, _A + 2, 1, 0, _A, 0, 1, 2, 3, 0, 1, 4, 8), "fp32 / int32 stream not 4-byte aligned"),
    ("mk_input_assemble_bwd", (_A, 0, None, None, None, 0, 0, _A + 2, 0, 1, 2, 3, 0, 0, 4, 8), "gradient not aligned to its element"),
    ("mk_input_assemble_bwd", (_A, 1, None, _A + 2, None, 0, 0, _A, 0, 1, 2, 3, 0, 0, 4, 8), "fp32 / int32 stream not 4-byte aligned"),
    ("mk_history_sums", (_A + 2, 0, None, _A, _A, _A, 1, 2, 3, 0, 4, 8), "x not aligned to its element"),
    ("mk_history_sums", (_A, 0, None, _A + 2, _A, _A, 1, 2, 3, 0, 4, 8), "fp32 stream not 4-byte aligned"),
    ("mk_history_sums", (_A, 1, _A, _A, _A + 4, _A, 1, 2, 3, 1, 4, 8), "fp64 buffer not 8-byte aligned"),
]


@pytest.mark.parametrize("case", MISALIGNED, ids=capi.case_ids(MISALIGNED))
def test_misaligned_pointer_is_refused_before_any_launch(case):
    capi.assert_refused(*case)
