"""GPU tests of the Lp training losses on the HIP kernels (lploss.hip through ops.geo_lp_sums, GeometricLpLoss and
LossHandler): every (p, absolute, squared) combination in fp32 and bf16 against the oracle and the closed-form gradient
(helpers and yardsticks of test_lploss_cpu.py), the production field, odd widths and unaligned streams, bitwise
determinism, spatial shards that add up, a captured forward + backward equal to the eager one bit for bit, and the C
ABI's argument checks.

Tolerances are the project's (test_kernels_gpu.py::test_geometric_l2_loss_fused_pass): loss 5e-6 relative, gradient 2e-6
relative L2.  For a bf16 prediction the expected values come from the bf16-rounded prediction and the gradient, stored
in bf16, gets 2^-9 on top (the worst-case rounding of one bf16 store).  Raw sums: 1e-6 per entry
(test_metrics_gpu.py)."""
import gc
import itertools

import pytest
import torch

from oracle import losses as ol
from test_lploss_cpu import SHAPE, closed_form, expected_loss, fields, make_params, no_ties, rel, sums64

pytestmark = pytest.mark.gpu

LOSS_TOL, GRAD_TOL, SUM_TOL = 5e-6, 2e-6, 1e-6
PROD = (73, 721, 1440)


def _grad_tol(dtype):
    return GRAD_TOL + (2.0 ** -9 if dtype == torch.bfloat16 else 0.0)


def _graph_names(fn):
    """Names of every autograd node reachable from ``fn``."""
    seen, todo, names = set(), [fn], set()
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.add(type(f).__name__)
        todo.extend(n for n, _ in f.next_functions)
    return names


def _rel_each(got, want):
    return ((got - want).abs() / want.abs()).max().item()


def _device_fields(dev, B, C, H, W, dtype, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    tar = torch.randn(B, C, H, W, device=dev, generator=g)
    prd = (0.8 * tar + 0.4 * torch.randn(B, C, H, W, device=dev, generator=g) + 0.1).to(dtype)
    wrow = torch.rand(H, device=dev, generator=g) + 0.1
    return prd, tar, wrow


def _check_loss(dev, loss, prd, tar, chw, q, dtype, **form):
    """Value against the oracle and gradient against the closed form, both from the prediction as stored in ``dtype``."""
    x = prd.to(dev).to(dtype).requires_grad_(True)
    seen = x.detach().float().cpu()                                    # what the kernel reads
    out = loss.to(dev)(x, tar.to(dev), chw.to(dev))
    out.backward()
    assert "_GeoLpSumsBackward" in _graph_names(out.grad_fn)
    assert out.dtype == torch.float32 and x.grad.dtype == dtype
    want = ol.geometric_lp_loss(seen.numpy(), tar.numpy(), chw.numpy(), q, **form)
    assert abs(float(out.detach()) - want) < LOSS_TOL * abs(want)
    gwant = closed_form(seen, tar, q, chw, form["p"], form["absolute"], form["squared"], form.get("size_average", False))[1]
    assert rel(x.grad.cpu(), gwant) < _grad_tol(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("p,absolute,squared", list(itertools.product([1, 2], [False, True], [False, True])))
def test_all_combinations_small(dev, p, absolute, squared, dtype):
    from makani_amd.losses import GeometricLpLoss
    B, C, H, W = SHAPE
    prd, tar = fields()
    assert no_ties(prd, tar)
    chw = torch.rand(1, C, generator=torch.Generator().manual_seed(6)) + 0.1
    kw = dict(img_shape=(H + 2, W + 3), crop_shape=(H, W), crop_offset=(1, 2))
    q = ol.quad_weight("legendre-gauss", kw["img_shape"], kw["crop_shape"], kw["crop_offset"], normalize=True, pole_mask=1)
    loss = GeometricLpLoss(p=p, absolute=absolute, squared=squared, pole_mask=1, quadrature_rule="legendre-gauss", **kw)
    _check_loss(dev, loss, prd, tar, chw, q, dtype, p=p, absolute=absolute, squared=squared)


def test_reductions_small(dev):
    from makani_amd.losses import GeometricLpLoss
    B, C, H, W = SHAPE
    prd, tar = fields()
    chw = torch.rand(1, C, generator=torch.Generator().manual_seed(6)) + 0.1
    kw = dict(img_shape=(H, W), crop_shape=(H, W), crop_offset=(0, 0))
    q = ol.quad_weight("naive", (H, W), (H, W), (0, 0), normalize=True)
    _check_loss(dev, GeometricLpLoss(p=1, size_average=True, **kw), prd, tar, chw, q, torch.float32, p=1, absolute=False,
                squared=False, size_average=True)
    per_loss = GeometricLpLoss(p=2, reduction=False, squared=True, **kw).to(dev)
    x = prd.to(dev).requires_grad_(True)
    per = per_loss(x, tar.to(dev), chw.to(dev))
    assert per.shape == (B, C) and per.dtype == torch.float32
    coef = torch.rand(B, C, generator=torch.Generator().manual_seed(7)) + 0.5
    (per * coef.to(dev)).sum().backward()
    want, gwant = closed_form(prd, tar, q, chw * coef, 2, False, True, reduction=False)
    assert rel(per.detach().cpu() * coef, want) < LOSS_TOL
    assert rel(x.grad.cpu(), gwant) < GRAD_TOL


@pytest.mark.parametrize("p,absolute,squared,dtype", [(2, False, False, torch.float32), (1, True, False, torch.bfloat16),
                                                      (2, False, True, torch.bfloat16)])
def test_production_field(dev, p, absolute, squared, dtype):
    """[1, 73, 721, 1440]: the value against the oracle on the host, the gradient against the closed form in float64 on
    the device."""
    from makani_amd.losses import GeometricLpLoss
    C, H, W = PROD
    g = torch.Generator(device=dev).manual_seed(12)
    tar = torch.randn(1, C, H, W, device=dev, generator=g)
    prd = torch.randn(1, C, H, W, device=dev, generator=g).to(dtype)
    assert int(((prd.float() - tar) == 0).sum()) == 0
    chw = (torch.rand(1, C, generator=torch.Generator().manual_seed(6)) + 0.1).to(dev)
    loss = GeometricLpLoss((H, W), (H, W), (0, 0), p=p, absolute=absolute, squared=squared,
                           quadrature_rule="legendre-gauss").to(dev)
    q = ol.quad_weight("legendre-gauss", (H, W), (H, W), (0, 0), normalize=True)
    x = prd.clone().requires_grad_(True)
    out = loss(x, tar, chw)
    out.backward()
    assert "_GeoLpSumsBackward" in _graph_names(out.grad_fn)
    want = ol.geometric_lp_loss(prd.float().cpu().numpy(), tar.cpu().numpy(), chw.cpu().numpy(), q, p=p, absolute=absolute,
                                squared=squared)
    assert abs(float(out.detach()) - want) < LOSS_TOL * abs(want)
    gwant = closed_form(prd.float(), tar, q, chw, p, absolute, squared)[1]
    assert x.grad.dtype == dtype and rel(x.grad, gwant) < _grad_tol(dtype)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("p", [1, 2])
def test_kernel_sums_production(dev, B, dtype, p):
    from makani_amd import ops
    prd, tar, wrow = _device_fields(dev, B, *PROD, dtype=dtype, seed=B)
    got = ops.geo_lp_sums(prd, tar, wrow, p)
    assert got.dtype == torch.float64 and got.shape == (B, PROD[0], 2)
    assert _rel_each(got, sums64(prd, tar, wrow, p)) < SUM_TOL


def _shift(x, offset):
    """A copy of x that starts ``offset`` elements into its allocation."""
    buf = torch.empty(x.numel() + offset, dtype=x.dtype, device=x.device)
    y = buf[offset:].view(x.shape)
    y.copy_(x)
    return y


@pytest.mark.parametrize("W", [1, 7, 61, 1441])
@pytest.mark.parametrize("offsets", [(0, 0), (1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("p", [1, 2])
def test_odd_widths_and_alignments(dev, W, offsets, dtype, p):
    """Rows that start off every 16-byte boundary, and a prediction / target that start one element (2 or 4 bytes) into
    an allocation: both shifted (rows vectorise behind a scalar head) or only one (rows run scalar)."""
    from makani_amd import ops
    B, C, H = 2, 3, 9
    prd, tar = fields((B, C, H, W), seed=12)
    assert no_ties(prd, tar)
    prd, tar = _shift(prd.to(dev).to(dtype), offsets[0]), _shift(tar.to(dev), offsets[1])
    assert (prd.data_ptr() % 16 != 0) == bool(offsets[0]) and (tar.data_ptr() % 16 != 0) == bool(offsets[1])
    wrow = torch.rand(H, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) + 0.1
    x = prd.detach().requires_grad_(True)
    assert x.data_ptr() == prd.data_ptr()
    got = ops.geo_lp_sums(x, tar, wrow, p)
    assert type(got.grad_fn).__name__ == "_GeoLpSumsBackward"
    assert _rel_each(got.detach(), sums64(prd, tar, wrow, p)) < SUM_TOL
    coef = torch.rand(B, C, 2, device=dev, generator=torch.Generator(device=dev).manual_seed(4)).double() + 0.5
    (coef * got).sum().backward()
    x64 = prd.double().requires_grad_(True)
    (coef[..., 0] * (wrow.double().view(1, 1, -1, 1) * (x64 - tar.double()).abs() ** p).sum((-2, -1))).sum().backward()
    assert x.grad.dtype == dtype and rel(x.grad, x64.grad) < _grad_tol(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("p", [1, 2])
def test_backward_into_an_unaligned_gradient(dev, dtype, p):
    """mk_geo_lp_bwd with prediction, target and gradient all one element into their allocations (the vector body behind
    a scalar head), into a guarded buffer: nothing is written outside the gradient."""
    from makani_amd import _lib, ops
    B, C, H, W = 2, 3, 9, 61
    prd, tar = fields((B, C, H, W), seed=12)
    prd, tar = _shift(prd.to(dev).to(dtype), 1), _shift(tar.to(dev), 1)
    wrow = torch.rand(H, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) + 0.1
    g = torch.rand(B, C, device=dev, generator=torch.Generator(device=dev).manual_seed(4)) + 0.5
    buf = torch.full((prd.numel() + 9,), 7.0, dtype=dtype, device=dev)
    gp = buf[1:1 + prd.numel()].view(prd.shape)
    _lib.check(_lib.load().mk_geo_lp_bwd(prd.data_ptr(), ops._pw_dtype(prd), tar.data_ptr(), wrow.data_ptr(), g.data_ptr(),
                                         gp.data_ptr(), p, B, C, H, W, torch.cuda.current_stream().cuda_stream))
    d = prd.double() - tar.double()
    want = g.double().view(B, C, 1, 1) * wrow.double().view(1, 1, H, 1) * (2.0 * d if p == 2 else torch.sign(d))
    assert rel(gp, want) < _grad_tol(dtype)
    assert float(buf[0]) == 7.0 and bool((buf[1 + prd.numel():] == 7.0).all())


def test_grad_fn_of_general_and_uniform_path(dev):
    from makani_amd.losses import GeometricLpLoss
    B, C, H, W = 2, 6, 48, 96
    prd, tar = fields((B, C, H, W))
    loss = GeometricLpLoss((H, W), (H, W), (0, 0), p=2, absolute=True, squared=True, quadrature_rule="legendre-gauss").to(dev)
    for chw, uniform in ((torch.full((1, C), 1.0 / C), 1.0 / C), (torch.rand(1, C) + 0.1, None)):
        loss.uniform_chw = uniform
        out = loss(prd.to(dev).requires_grad_(True), tar.to(dev), chw.to(dev))
        names = _graph_names(out.grad_fn)
        if uniform is not None:
            assert type(out.grad_fn).__name__ == "_WeightedMSEBackward" and "_GeoLpSumsBackward" not in names
        else:
            assert "_GeoLpSumsBackward" in names and "_WeightedMSEBackward" not in names
            # nothing but the sums touches the fields: no elementwise torch op on [B, C, H, W]
            assert not names & {"AbsBackward0", "SubBackward0", "PowBackward0"}


@pytest.mark.parametrize("p", [1, 2])
def test_bitwise_repeatable(dev, p):
    from makani_amd import ops
    prd, tar, wrow = _device_fields(dev, 2, *PROD, dtype=torch.bfloat16, seed=9)
    coef = torch.rand(2, PROD[0], 2, device=dev, dtype=torch.float64) + 0.5
    runs = []
    for _ in range(2):
        x = prd.clone().requires_grad_(True)
        s = ops.geo_lp_sums(x, tar, wrow, p)
        (coef * s).sum().backward()
        runs.append((s.detach(), x.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("axis,shapes", [("h", [181, 181, 181, 178]), ("w", [180] * 8)])
@pytest.mark.parametrize("p", [1, 2])
def test_shard_sums_add_up(dev, axis, shapes, p):
    from makani_amd import ops
    from makani_amd.distributed import compute_split_shapes
    prd, tar, wrow = _device_fields(dev, 1, *PROD, dtype=torch.float32, seed=11)
    full = ops.geo_lp_sums(prd, tar, wrow, p)
    assert compute_split_shapes(PROD[1] if axis == "h" else PROD[2], len(shapes)) == shapes
    total = torch.zeros_like(full)
    o = 0
    for n in shapes:
        if axis == "h":
            part = ops.geo_lp_sums(prd[:, :, o:o + n].contiguous(), tar[:, :, o:o + n].contiguous(),
                                   wrow[o:o + n].contiguous(), p)
        else:
            part = ops.geo_lp_sums(prd[..., o:o + n].contiguous(), tar[..., o:o + n].contiguous(), wrow, p)
        total += part
        o += n
    assert _rel_each(total, full) < SUM_TOL


@pytest.mark.parametrize("spec", ["weighted squared geometric l2", "weighted pole-masked geometric l2"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_loss_handler_on_the_kernels(dev, spec, dtype):
    from makani_amd.losses import LossHandler
    B, C, H, W = SHAPE
    params = make_params(spec, H, W, n_future=1, img_shape=(H + 2, W + 3), crop_offset=(1, 2), grid="legendre_gauss")
    prd, tar = fields((B, 2 * C, H, W))
    handler = LossHandler(params).to(dev)
    handler.train()
    x = prd.to(dev).to(dtype).requires_grad_(True)
    out = handler(x, tar.to(dev), None)
    out.backward()
    assert "_GeoLpSumsBackward" in _graph_names(out.grad_fn)
    want, gwant = expected_loss(params, x.detach().float().cpu(), tar, True)
    assert abs(float(out.detach()) - want) < LOSS_TOL * abs(want)
    assert rel(x.grad.cpu(), gwant) < _grad_tol(dtype)


def test_captured_loss_matches_eager_bitwise(dev):
    """LossHandler forward + backward (unequal channel weights) in one graph, replayed on new inputs."""
    from makani_amd.losses import LossHandler
    B, C, H, W = 2, 6, 90, 180
    handler = LossHandler(make_params("weighted squared geometric l2", H, W)).to(dev)
    handler.train()
    inputs = [tuple(t.to(dev) for t in fields((B, C, H, W), seed=s)) for s in (12, 13, 14)]
    inputs = [(p.bfloat16(), t) for p, t in inputs]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = []
        for p, t in inputs:
            x = p.clone().requires_grad_(True)
            loss = handler(x, t, None)
            loss.backward()
            eager.append((loss.detach().clone(), x.grad.clone()))
            del loss, x
        static_prd = inputs[0][0].clone().requires_grad_(True)
        static_tar = inputs[0][1].clone()
        for _ in range(2):                                             # warm-ups on the capture stream
            static_prd.grad = None
            handler(static_prd, static_tar, None).backward()
        static_prd.grad = None
        gc.collect()
        torch.cuda.empty_cache()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            static_loss = handler(static_prd, static_tar, None)
            static_loss.backward()
        for (p, t), (want_loss, want_grad) in zip(inputs[1:] + inputs[:1], eager[1:] + eager[:1]):
            with torch.no_grad():
                static_prd.copy_(p)
                static_tar.copy_(t)
            graph.replay()
            side.synchronize()
            assert torch.equal(static_loss.detach(), want_loss) and torch.equal(static_prd.grad, want_grad)
    torch.cuda.current_stream().wait_stream(side)
    assert not torch.equal(eager[0][1], eager[1][1])


def test_c_abi_rejects_bad_arguments(dev):
    """Bad arguments come back non-zero with a message from the host-side checks, before any launch."""
    from makani_amd import _lib
    lib = _lib.load()
    B, C, H, W = 1, 2, 5, 8
    prd = torch.randn(B, C, H, W, device=dev)
    tar, gp = torch.randn_like(prd), torch.full_like(prd, 3.0)
    wrow, g = torch.ones(H, device=dev), torch.ones(B, C, device=dev)
    ws = torch.zeros(lib.mk_geo_lp_workspace(B, C, H), dtype=torch.float64, device=dev)
    out = torch.full((B, C, 2), -1.0, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    a = (prd.data_ptr(), 0, tar.data_ptr(), wrow.data_ptr())

    def fwd(args=a, ws_=ws.data_ptr(), out_=out.data_ptr(), p=2, W_=W):
        return lib.mk_geo_lp_sums(*args, ws_, out_, p, B, C, H, W_, st)

    def bwd(args=a, g_=g.data_ptr(), gp_=gp.data_ptr(), p=2, W_=W):
        return lib.mk_geo_lp_bwd(*args, g_, gp_, p, B, C, H, W_, st)

    for call, needle in ((lambda: fwd(p=3), b"p must be 1 or 2"), (lambda: bwd(p=3), b"p must be 1 or 2"),
                         (lambda: fwd(p=0), b"p must be 1 or 2"),
                         (lambda: fwd(args=(None,) + a[1:]), b"null pointer"), (lambda: fwd(out_=None), b"null pointer"),
                         (lambda: bwd(gp_=None), b"null pointer"), (lambda: bwd(g_=None), b"null pointer"),
                         (lambda: fwd(W_=0), b"bad sizes"), (lambda: bwd(W_=0), b"bad sizes"),
                         (lambda: fwd(args=(a[0], 2) + a[2:]), b"dtype")):
        assert call() != 0
        assert needle in lib.mk_last_error()
    assert lib.mk_geo_lp_workspace(0, C, H) == 0
    torch.cuda.synchronize()
    assert bool((out == -1.0).all()) and bool((gp == 3.0).all())        # nothing was launched
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert bool((out > 0).all())
