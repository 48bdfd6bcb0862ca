"""GPU tests of the one-pass input assembly (csrc/preproc.hip) and of the step wrappers on it.

The yardstick is ``Preprocessor2D._assemble_torch`` -- the reference's composition in torch ops -- on the same device
tensors, and the CPU path.  Assembly in mode "none" is copies and one fp32 product, the normalisation a subtraction and
a correctly rounded fp32 division: the HIP pass must equal the torch formulation bit for bit, forward and backward, in
fp32, and its bf16 output the fp32 output's ``.to(bfloat16)``.  The statistics come from fp64 sums: mean and std within
1e-6 of float64 (the mean relative to the std), bitwise repeatable.

The captured-step test uses a toy model made of torch's deterministic elementwise and reduction kernels, so that loss
and parameter gradients can be compared bit for bit; with the package's SFNO the loss is compared bit for bit and the
parameter gradients to 1e-3 as in test_model_gpu.py, because the net's 1x1-convolution weight gradients are summed with
fp32 atomics (test_optim_gpu.py) and differ in their last bits from run to run with or without a graph."""
import gc
import itertools

import numpy as np
import pytest
import torch

from test_lploss_gpu import _graph_names
from test_stepper_cpu import FIELD_TOL, STAT_TOL, make_params, rel, scaled_fields, stats_f64

pytestmark = pytest.mark.gpu

PROD = (73, 1, 721, 1440)         # predicted, unpredicted channels, grid of the reference's configs (35 static channels)


def _static_kw(tmp_path, H, W, Cs):
    """Constructor arguments that give ``Cs`` static channels: 3 = linear grid + orography, 35 = 16 sinusoidal
    frequencies + orography + land mask (the production set)."""
    if Cs == 0:
        return {}
    g = torch.Generator().manual_seed(100 + H + W)
    oro, lsm = tmp_path / f"oro_{H}x{W}.npy", tmp_path / f"lsm_{H}x{W}.npy"
    if not oro.exists():
        np.save(oro, (3000.0 * torch.rand(H, W, generator=g)).numpy())
        np.save(lsm, (torch.rand(H, W, generator=g) > 0.6).numpy().astype(np.int64))
    if Cs == 3:
        return dict(add_grid=True, gridtype="linear", add_orography=True, orography_path=str(oro))
    assert Cs == 35
    return dict(add_grid=True, gridtype="sinusoidal", grid_num_frequencies=16, add_orography=True, orography_path=str(oro),
                add_landmask=True, landmask_path=str(lsm))


def _offset(t, off):
    """``t``'s values in a storage that starts ``off`` elements into an allocation."""
    if off == 0:
        return t
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)
    out = buf[off:].view(t.shape)
    out.copy_(t)
    assert out.storage_offset() == off
    return out


def _setup(dev, tmp_path, B, T, C, Cu, Cs, H, W, mode="none", masked=(), seed=0, off=0, train=False):
    from makani_amd.preprocessor import Preprocessor2D
    pp = Preprocessor2D(make_params(H, W, n_history=T - 1, history_normalization_mode=mode, masked_channels=list(masked),
                                    **_static_kw(tmp_path, H, W, Cs))).to(dev)
    pp.train(train)
    xa = scaled_fields((B, T, C + Cu, H, W), seed=seed).to(dev)
    x = _offset(xa[:, :, :C].reshape(B, T * C, H, W).contiguous(), off)
    u = _offset(xa[:, :, C:].contiguous(), off) if Cu else None
    pp.cache_unpredicted_features(None, None, u, None)
    assert (pp.static_features.shape[1] if Cs else 0) == Cs
    return pp, x, u, xa


def _to_cpu(pp, u):
    import copy
    cp = copy.deepcopy(pp).cpu()
    cp._mask_cache = {}
    cp.history_mean = cp.history_std = None
    cp.unpredicted_inp_train = cp.unpredicted_tar_train = cp.unpredicted_inp_eval = cp.unpredicted_tar_eval = None
    cp.cache_unpredicted_features(None, None, u.cpu() if u is not None else None, None)
    return cp


# ---------------------------------------------------------------------------- assembly, bit-equality
@pytest.mark.parametrize("W", [60, 61, 1440])
@pytest.mark.parametrize("B", [1, 2])
def test_assembly_equals_torch_bitwise(dev, tmp_path, W, B):
    H, C = 6, 4
    n = 0
    for T, Cu, Cs, mask, off in itertools.product((1, 2), (0, 1), (0, 3, 35), (False, True), (0, 1)):
        if mask and Cs == 0:
            continue                                   # the mask is a static channel
        if T == 1 and Cu == 0 and Cs == 0:
            continue                                   # nothing to do: checked in test_nothing_to_do_launches_nothing
        pp, x, u, _ = _setup(dev, tmp_path, B, T, C, Cu, Cs, H, W, masked=(1, 3) if mask else (), seed=n, off=off)
        want = pp._assemble_torch(x)
        got = pp.assemble(x)
        what = (T, Cu, Cs, mask, off)
        assert got.shape == (B, T * (C + Cu) + Cs, H, W) and got.dtype == torch.float32, what
        assert torch.equal(got, want), what
        assert torch.equal(pp.assemble(x, out_dtype=torch.bfloat16), want.to(torch.bfloat16)), what
        xb = x.to(torch.bfloat16)
        assert torch.equal(pp.assemble(xb), pp.assemble(xb.float())), what
        assert torch.equal(pp.assemble(xb, out_dtype=torch.bfloat16), pp._assemble_torch(xb, torch.bfloat16)), what
        if off == 0:
            assert torch.equal(got.cpu(), _to_cpu(pp, u)._assemble_torch(x.cpu())), what
        n += 1
    assert n == 2 * (2 * 2 * 3 + 2 * 2 * 2) - 2 * 1


@pytest.mark.parametrize("B", [1, 2])
def test_production_shape(dev, tmp_path, B):
    C, Cu, H, W = PROD
    pp, x, u, _ = _setup(dev, tmp_path, B, 1, C, Cu, 35, H, W, masked=(20,), seed=7)
    want = pp._assemble_torch(x)
    got = pp.assemble(x)
    assert got.shape == (B, 109, H, W)
    assert torch.equal(got, want)
    del got
    assert torch.equal(pp.assemble(x, out_dtype=torch.bfloat16), want.to(torch.bfloat16))
    assert not torch.equal(want[:, 20], x[:, 20]) and torch.equal(want[:, 21], x[:, 21])


def test_nothing_to_do_launches_nothing(dev):
    from makani_amd.preprocessor import Preprocessor2D
    pp = Preprocessor2D(make_params(6, 8)).to(dev)
    x = torch.randn(2, 3, 6, 8, device=dev)
    assert pp.assemble(x) is x


# ---------------------------------------------------------------------------- statistics modes
@pytest.mark.parametrize("mode", ["exponential", "mean"])
@pytest.mark.parametrize("shape", [(2, 3, 4, 1, 7, 61, 1), (2, 2, 4, 0, 33, 60, 0), (1, 1, 73, 1, 721, 1440, 0),
                                   (2, 2, 6, 1, 91, 180, 0)])
def test_statistics_modes(dev, tmp_path, mode, shape):
    from makani_amd import ops
    B, T, C, Cu, H, W, off = shape
    pp, x, u, xa = _setup(dev, tmp_path, B, T, C, Cu, 3, H, W, mode=mode, masked=(2,), seed=H, off=off)
    got = pp.assemble(x)
    mean, std = pp.history_mean, pp.history_std
    assert mean.shape == (B, C + Cu, 1, 1) and mean.dtype == torch.float32 and std.dtype == torch.float32
    m64, s64 = stats_f64(xa, pp.history_normalization_weights, H * W)
    em = ((mean.double() - m64).abs() / s64).max().item()
    es = ((std.double() - s64).abs() / s64).max().item()
    print(f"{mode} {shape}: mean err / std {em:.2e}, std rel err {es:.2e} (bound {STAT_TOL:.0e})")
    assert em < STAT_TOL and es < STAT_TOL
    # the field: torch's fp32 arithmetic on the kernel's own statistics, bit for bit
    Cd = T * (C + Cu)
    want = ((xa - mean.unsqueeze(1)) / std.unsqueeze(1)).reshape(B, Cd, H, W)
    want[:, [t * (C + Cu) + 2 for t in range(T)]] *= pp.static_features[:, -1:]
    assert torch.equal(got[:, :Cd], want)
    assert torch.equal(got[:, Cd:], pp.static_features.expand(B, -1, -1, -1))
    assert rel(got[:, :Cd], pp._assemble_torch(x)[:, :Cd]) < FIELD_TOL
    assert torch.equal(pp.assemble(x, out_dtype=torch.bfloat16), got.to(torch.bfloat16))
    # two calls are bitwise identical, sums included
    wt = pp.history_normalization_weights.reshape(-1)
    x5 = pp.expand_history(x, T)
    s1, s2 = ops.history_sums(x5, u, wt), ops.history_sums(x5, u, wt)
    assert s1.dtype == torch.float64 and s1.shape == (B, C + Cu, 2) and torch.equal(s1, s2)
    assert torch.equal(pp.assemble(x), got) and torch.equal(pp.history_mean, mean) and torch.equal(pp.history_std, std)
    # the sums against torch float64 on the device, and a bf16 history read as it is
    ref = ops._history_sums_torch(xa, wt)
    assert ((s1[..., 1] - ref[..., 1]).abs() / ref[..., 1]).max() < 1e-12
    assert ((s1[..., 0] - ref[..., 0]).abs() / (ref[..., 1] * (H * W)).sqrt()).max() < 1e-12       # Cauchy-Schwarz scale
    # a bf16 history is read as it is: the same values as its fp32 copy, summed in another order (a bf16 row has
    # another 16-byte boundary), so equal to fp64 rounding
    xb = x5.to(torch.bfloat16)
    sb, sf = ops.history_sums(xb, u, wt), ops.history_sums(xb.float(), u, wt)
    assert ((sb[..., 1] - sf[..., 1]).abs() / sf[..., 1]).max() < 1e-12
    assert ((sb[..., 0] - sf[..., 0]).abs() / (sf[..., 1] * (H * W)).sqrt()).max() < 1e-12
    # history_compute_stats on its own takes the same kernel on the concatenated tensor (other row alignments, so
    # another summation order: equal to rounding, not bitwise)
    pp.history_compute_stats(pp.append_unpredicted_features(x))
    assert ((pp.history_mean - mean).abs() / std).max() < STAT_TOL and ((pp.history_std - std).abs() / std).max() < STAT_TOL


# ---------------------------------------------------------------------------- backward
@pytest.mark.parametrize("W", [61, 64])
@pytest.mark.parametrize("x_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("g_dtype", [torch.float32, torch.bfloat16])
def test_backward_mode_none_equals_autograd_bitwise(dev, tmp_path, W, x_dtype, g_dtype):
    B, T, C, Cu, Cs, H = 2, 2, 4, 1, 3, 7
    for mask, off in itertools.product((False, True), (0, 1)):
        pp, x, u, _ = _setup(dev, tmp_path, B, T, C, Cu, Cs, H, W, masked=(0, 3) if mask else (), seed=3, off=off, train=True)
        x = _offset(x.to(x_dtype), off)
        cot = torch.randn(B, T * (C + Cu) + Cs, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(4)).to(g_dtype)
        a = _offset(x.clone(), off).requires_grad_(True)
        assert a.is_leaf and a.storage_offset() == off
        out = pp.assemble(a, out_dtype=g_dtype)
        assert "_InputAssembleBackward" in _graph_names(out.grad_fn)
        out.backward(cot)
        b = x.clone().requires_grad_(True)
        ref = pp._assemble_torch(b, out_dtype=g_dtype)
        assert "_InputAssembleBackward" not in _graph_names(ref.grad_fn)
        ref.backward(cot)
        assert torch.equal(out, ref)
        assert a.grad.dtype == x_dtype and a.grad.shape == x.shape
        assert torch.equal(a.grad, b.grad), (mask, off)
        if mask:
            assert not torch.equal(a.grad[:, 0].float(), cot[:, 0].float())


def test_statistics_mode_with_gradient_takes_the_torch_path(dev, tmp_path):
    B, T, C, Cu, H, W = 2, 2, 4, 1, 9, 16
    pp, x, u, xa = _setup(dev, tmp_path, B, T, C, Cu, 3, H, W, mode="exponential", seed=5, train=True)
    a = x.clone().requires_grad_(True)
    out = pp.assemble(a)
    names = _graph_names(out.grad_fn)
    assert "_InputAssembleBackward" not in names and "CatBackward0" in names
    cot = torch.randn_like(out)
    out.backward(cot)
    # the gradient through the statistics: float64 autograd of the definition
    x64 = xa.double().clone().requires_grad_(True)
    w = pp.history_normalization_weights.double()
    m = (x64 * w).sum((1, 3, 4), keepdim=True) / (H * W)
    s = (((x64 - m) ** 2 * w).sum((1, 3, 4), keepdim=True) / (H * W)).sqrt()
    Cd = T * (C + Cu)
    (((x64 - m) / s).reshape(B, Cd, H, W) * cot[:, :Cd].double()).sum().backward()
    assert rel(a.grad, x64.grad[:, :, :C].reshape(B, T * C, H, W)) < 1e-5
    # without a gradient the same call is the HIP pass; with the statistics as constants the op's own backward
    with torch.no_grad():
        assert pp.assemble(x).grad_fn is None
    from makani_amd import ops
    mean, std = pp.history_mean.detach(), pp.history_std.detach()
    c = x.clone().requires_grad_(True)
    o = ops.input_assemble(pp.expand_history(c, T), u, pp.static_features[0], mean, std)
    assert type(o.grad_fn).__name__ == "_InputAssembleBackward"
    o.backward(cot)
    want = (cot[:, :Cd].reshape(B, T, C + Cu, H, W) / std.unsqueeze(1))[:, :, :C].reshape(B, T * C, H, W)
    assert torch.equal(c.grad, want)


# ---------------------------------------------------------------------------- wrappers
def _sfno(dev, cin, cout, H=64, W=128, seed=11):
    from makani_amd.sfnonet import SphericalFourierNeuralOperatorNet
    torch.manual_seed(seed)
    kw = dict(inp_shape=(H, W), out_shape=(H, W), scale_factor=2, inp_chans=cin, out_chans=cout, embed_dim=16, num_layers=2,
              big_skip=True)
    return lambda: SphericalFourierNeuralOperatorNet(**kw)


@pytest.mark.parametrize("single", [True, False])
def test_wrappers_feed_the_engine_bf16_field_directly(dev, single):
    from makani_amd import stepper
    H, W, B, T, C, Cu = 64, 128, 2, 2, 3, 1
    p = make_params(H, W, n_history=T - 1, add_grid=True, n_future=0)
    cls = stepper.SingleStepWrapper if single else stepper.MultiStepWrapper
    wrap = cls(p, _sfno(dev, T * (C + Cu) + 4, C)).to(dev)
    wrap.eval()
    g = torch.Generator(device=dev).manual_seed(2)
    inp, xz = torch.randn(B, T * C, H, W, device=dev, generator=g), torch.randn(B, T, Cu, H, W, device=dev, generator=g)
    wrap.preprocessor.cache_unpredicted_features(None, None, xz, None)
    seen = []
    assemble = wrap.preprocessor.assemble
    wrap.preprocessor.assemble = lambda x, out_dtype=None: seen.append(out_dtype) or assemble(x, out_dtype)
    with torch.no_grad():
        assert stepper._engine_input_dtype(wrap.model, inp) is None           # no autocast: fp32
        y32 = wrap(inp)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = wrap(inp)
            want = wrap.model(assemble(inp))                                 # the model fed the fp32 assembly
    assert seen == [None, torch.bfloat16]
    assert torch.equal(y, want) and y.shape == (B, C, H, W)
    assert torch.isfinite(y).all() and torch.isfinite(y32).all() and y32.dtype == torch.float32


def test_eval_rollout_equals_the_torch_formulation_bitwise(dev):
    from makani_amd.stepper import MultiStepWrapper
    H, W, B, T, C, Cu, steps = 64, 128, 2, 2, 3, 1, 3
    p = make_params(H, W, n_history=T - 1, add_grid=True, n_future=0, masked_channels=[1])
    wrap = MultiStepWrapper(p, _sfno(dev, T * (C + Cu) + 4, C)).to(dev)
    wrap.eval()
    g = torch.Generator(device=dev).manual_seed(3)
    inp, xz = torch.randn(B, T * C, H, W, device=dev, generator=g), torch.randn(B, T, Cu, H, W, device=dev, generator=g)
    yz = torch.randn(B, steps, Cu, H, W, device=dev, generator=g)

    def rollout():
        wrap.preprocessor.cache_unpredicted_features(None, None, xz.clone(), yz.clone())
        outs, x = [], inp
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            for step in range(steps):
                y = wrap(x)
                outs.append(y)
                x = wrap.preprocessor.append_history(x, y, step)
        return outs, wrap.preprocessor.unpredicted_inp_eval.clone()

    hip, u_hip = rollout()
    wrap.preprocessor.assemble = wrap.preprocessor._assemble_torch
    ref, u_ref = rollout()
    for a, b in zip(hip, ref):
        assert torch.equal(a, b)
    assert torch.equal(u_hip, u_ref) and torch.equal(u_hip[:, -1], yz[:, steps - 1])
    assert not torch.equal(hip[0], hip[1]) and not torch.equal(hip[1], hip[2])


# ---------------------------------------------------------------------------- graph capture
class _ToyModel(torch.nn.Module):
    """A channel mix made of elementwise products and torch reductions only: deterministic gradients."""

    def __init__(self, cin, cout):
        super().__init__()
        g = torch.Generator().manual_seed(17)
        self.weight = torch.nn.Parameter(torch.randn(cout, cin, generator=g) / cin ** 0.5)
        self.bias = torch.nn.Parameter(torch.randn(cout, generator=g))

    def forward(self, x):
        return (x.float().unsqueeze(1) * self.weight[None, :, :, None, None]).sum(2) + self.bias[None, :, None, None]


def _captured_step(dev, model_handle, autocast, H, W):
    """MultiStepWrapper train forward (n_future = 1) + LossHandler + backward: eager results on three inputs, then one
    capture replayed on them.  Returns [(loss, parameter gradients)] for eager and for the replays."""
    from makani_amd.losses import LossHandler
    from makani_amd.stepper import MultiStepWrapper
    from test_lploss_cpu import make_params as loss_params
    B, T, C, Cu = 2, 2, 6, 1
    wrap = MultiStepWrapper(make_params(H, W, n_history=T - 1, add_grid=True, n_future=1, masked_channels=[2]), model_handle).to(dev)
    handler = LossHandler(loss_params("weighted squared geometric l2", H, W, n_future=1)).to(dev)
    wrap.train()
    handler.train()
    g = torch.Generator(device=dev).manual_seed(8)

    def batch():
        return (torch.randn(B, T * C, H, W, device=dev, generator=g), torch.randn(B, 2 * C, H, W, device=dev, generator=g),
                torch.randn(B, T, Cu, H, W, device=dev, generator=g), torch.randn(B, 2, Cu, H, W, device=dev, generator=g))

    batches = [batch() for _ in range(3)]
    static = [t.clone() for t in batches[0]]
    params = list(wrap.parameters())

    def load(b):
        with torch.no_grad():
            for s, t in zip(static[:2], b[:2]):
                s.copy_(t)
        wrap.preprocessor.cache_unpredicted_features(None, None, b[2], b[3])     # copies into the cached (static) tensors

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            prd = wrap(static[0])
        loss = handler(prd, static[1], None)
        loss.backward()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        wrap.preprocessor.cache_unpredicted_features(None, None, static[2], static[3])
        eager = []
        for b in batches:
            load(b)
            wrap.zero_grad(set_to_none=True)
            loss = step()
            eager.append((loss.detach().clone(), [q.grad.clone() for q in params]))
            del loss
        wrap.zero_grad(set_to_none=True)
        load(batches[0])
        gc.collect()
        torch.cuda.empty_cache()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            static_loss = step()
        replayed = []
        for b in batches[1:] + batches[:1]:
            load(b)
            graph.replay()
            side.synchronize()
            replayed.append((static_loss.detach().clone(), [q.grad.clone() for q in params]))
    torch.cuda.current_stream().wait_stream(side)
    return eager[1:] + eager[:1], replayed


def test_captured_multistep_training_step_matches_eager_bitwise(dev):
    H, W = 30, 61
    eager, replayed = _captured_step(dev, lambda: _ToyModel(2 * 7 + 4, 6), False, H, W)
    for (le, ge), (lr_, gr) in zip(eager, replayed):
        assert torch.equal(le, lr_)
        for a, b in zip(ge, gr):
            assert torch.equal(a, b)
    assert not torch.equal(eager[0][0], eager[1][0])


def test_captured_multistep_training_step_with_the_sfno(dev):
    H, W = 64, 128
    eager, replayed = _captured_step(dev, _sfno(dev, 2 * 7 + 4, 6, H, W), True, H, W)
    for (le, ge), (lr_, gr) in zip(eager, replayed):
        assert torch.equal(le, lr_)                   # the forward has no atomics
        for a, b in zip(ge, gr):
            a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
            # a gradient that vanishes identically (a bias in front of a normalisation) is an exact zero in both
            assert torch.isfinite(b).all() and (b - a).norm() <= 1e-3 * a.norm(), (a.shape, float(a.norm()))
    assert not torch.equal(eager[0][0], eager[1][0])


# ---------------------------------------------------------------------------- C ABI
def test_c_abi_rejects_bad_arguments(dev):
    """Bad arguments come back non-zero with a message from the host-side checks, before any launch."""
    from makani_amd import _lib
    lib = _lib.load()
    B, T, C, Cu, Cs, H, W = 1, 2, 3, 1, 2, 5, 8
    Ct = T * (C + Cu) + Cs
    x, u, stat = torch.randn(B, T, C, H, W, device=dev), torch.randn(B, T, Cu, H, W, device=dev), torch.randn(Cs, H, W, device=dev)
    mean, std = torch.zeros(B, C + Cu, device=dev), torch.ones(B, C + Cu, device=dev)
    mask = torch.tensor([1], dtype=torch.int32, device=dev)
    out = torch.full((B, Ct, H, W), 3.0, device=dev)
    gx = torch.full((B, T, C, H, W), 3.0, device=dev)
    wt = torch.ones(T, device=dev)
    ws = torch.zeros(lib.mk_history_workspace(B, C + Cu, H), dtype=torch.float64, device=dev)
    sums = torch.full((B, C + Cu, 2), -1.0, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    dims = (B, T, C, Cu, Cs, H, W)

    def fwd(x_=x.data_ptr(), xd=0, u_=u.data_ptr(), stat_=stat.data_ptr(), mean_=mean.data_ptr(), std_=std.data_ptr(),
            mask_=mask.data_ptr(), n_mask=1, src=Cs - 1, out_=out.data_ptr(), od=0, dims_=dims):
        return lib.mk_input_assemble(x_, xd, u_, stat_, mean_, std_, mask_, n_mask, src, out_, od, *dims_, st)

    def bwd(g_=out.data_ptr(), gd=0, stat_=stat.data_ptr(), std_=std.data_ptr(), mask_=mask.data_ptr(), n_mask=1, src=Cs - 1,
            gx_=gx.data_ptr(), xd=0, dims_=dims):
        return lib.mk_input_assemble_bwd(g_, gd, stat_, std_, mask_, n_mask, src, gx_, xd, *dims_, st)

    def hsum(x_=x.data_ptr(), xd=0, u_=u.data_ptr(), wt_=wt.data_ptr(), ws_=ws.data_ptr(), sums_=sums.data_ptr(), W_=W):
        return lib.mk_history_sums(x_, xd, u_, wt_, ws_, sums_, B, T, C, Cu, H, W_, st)

    for call, needle in ((lambda: fwd(x_=None), b"null pointer"), (lambda: fwd(out_=None), b"null pointer"),
                         (lambda: fwd(mask_=None), b"null pointer"), (lambda: fwd(u_=None), b"u must be given"),
                         (lambda: fwd(stat_=None), b"stat must be given"), (lambda: fwd(std_=None), b"mean and std"),
                         (lambda: fwd(xd=2), b"dtype"), (lambda: fwd(od=-1), b"dtype"),
                         (lambda: fwd(src=Cs), b"mask source"), (lambda: fwd(src=-1), b"mask source"),
                         (lambda: fwd(n_mask=-1), b"masked channels"), (lambda: fwd(dims_=dims[:-1] + (0,)), b"bad sizes"),
                         (lambda: bwd(g_=None), b"null pointer"), (lambda: bwd(gx_=None), b"null pointer"),
                         (lambda: bwd(mask_=None), b"null pointer"), (lambda: bwd(gd=2), b"dtype"), (lambda: bwd(xd=7), b"dtype"),
                         (lambda: bwd(src=Cs), b"mask source"), (lambda: bwd(dims_=(0,) + dims[1:]), b"bad sizes"),
                         (lambda: hsum(x_=None), b"null pointer"), (lambda: hsum(wt_=None), b"null pointer"),
                         (lambda: hsum(sums_=None), b"null pointer"), (lambda: hsum(u_=None), b"u must be given"),
                         (lambda: hsum(xd=3), b"dtype"), (lambda: hsum(W_=0), b"bad sizes")):
        assert call() != 0
        assert needle in lib.mk_last_error(), (needle, lib.mk_last_error())
    assert lib.mk_history_workspace(0, C, H) == 0
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((gx == 3.0).all()) and bool((sums == -1.0).all())     # nothing was launched
    assert fwd() == 0 and bwd() == 0 and hsum() == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:, Ct - Cs:], stat.unsqueeze(0))
    # a masked-channel entry outside the dynamic channels matches no row
    far = torch.tensor([Ct + 5], dtype=torch.int32, device=dev)
    assert fwd(mask_=far.data_ptr(), mean_=None, std_=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:, :C], x[:, 0])
