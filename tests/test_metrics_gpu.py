"""GPU tests of the validation-metric kernel (metrics.hip through ops.geo_metric_sums) and of MetricsHandler on the
device: the five sums against torch float64 on the production field, odd shapes and alignments, bitwise determinism,
spatial shards that add up to the full field, a captured rollout equal to the eager one bit for bit, and the handler's
logs against the float64 restatement of test_metrics_cpu.py."""
import pytest
import torch

from test_metrics_cpu import CHANNELS, check_handler, make_params, make_rollout, rel, run_handler

pytestmark = pytest.mark.gpu

PROD = (73, 721, 1440)


def _fields(dev, B, C, H, W, dtype=torch.float32, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    clim = 0.5 * torch.randn(C, H, W, device=dev, generator=g)
    tar = clim + torch.randn(B, C, H, W, device=dev, generator=g)
    prd = (0.8 * tar + 0.4 * torch.randn(B, C, H, W, device=dev, generator=g) + 0.1).to(dtype)
    wrow = torch.rand(H, device=dev, generator=g) + 0.1
    return prd, tar, clim, wrow


def _sums64(prd, tar, clim, wrow):
    """torch float64 on the device, one sample at a time: [B, C, 5]."""
    w = wrow.double().view(1, -1, 1)
    c = clim.double() if clim is not None else torch.zeros((), dtype=torch.float64, device=prd.device)
    out = []
    for b in range(prd.shape[0]):
        p, t = prd[b].double(), tar[b].double()
        d, pa, ta = p - t, p - c, t - c
        out.append(torch.stack([(w * d.abs()).sum((-2, -1)), (w * d * d).sum((-2, -1)), (w * pa * ta).sum((-2, -1)),
                                (w * pa * pa).sum((-2, -1)), (w * ta * ta).sum((-2, -1))], dim=-1))
        del p, t, d, pa, ta
    return torch.stack(out)


def _rel_each(got, want):
    return ((got - want).abs() / want.abs()).max().item()


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_clim", [True, False])
def test_kernel_sums_production(dev, B, dtype, with_clim):
    from makani_amd import ops
    prd, tar, clim, wrow = _fields(dev, B, *PROD, dtype=dtype, seed=B)
    clim = clim if with_clim else None
    got = ops.geo_metric_sums(prd, tar, clim, wrow)
    assert got.dtype == torch.float64 and got.shape == (B, PROD[0], 5)
    assert _rel_each(got, _sums64(prd, tar, clim, wrow)) < 1e-6


def test_kernel_sums_cropped_window(dev):
    from makani_amd import ops
    prd, tar, clim, wrow = _fields(dev, 1, *PROD, seed=3)
    win = (slice(None), slice(None), slice(1, 721), slice(None))
    got = ops.geo_metric_sums(prd[win], tar[win], clim[:, 1:721], wrow[1:721])
    assert _rel_each(got, _sums64(prd[win], tar[win], clim[:, 1:721], wrow[1:721])) < 1e-6


@pytest.mark.parametrize("W,offset", [(180, 0), (37, 1), (1440, 3)])
def test_kernel_sums_odd_widths_and_alignments(dev, W, offset):
    """bf16 180 wide (rows not 16-byte aligned), an odd width and buffers starting off any 16-byte boundary."""
    from makani_amd import ops
    B, C, H = 2, 73, 721 if W == 180 else 45
    prd, tar, clim, wrow = _fields(dev, B, C, H, W, dtype=torch.bfloat16, seed=W)
    if offset:
        def shift(x):
            buf = torch.empty(x.numel() + offset, dtype=x.dtype, device=dev)
            y = buf[offset:].view(x.shape)
            y.copy_(x)
            return y
        prd, tar, clim = shift(prd), shift(tar), shift(clim)
        assert prd.data_ptr() % 16 != 0 and tar.data_ptr() % 16 != 0
    got = ops.geo_metric_sums(prd, tar, clim, wrow)
    assert _rel_each(got, _sums64(prd, tar, clim, wrow)) < 1e-6


def test_kernel_sums_deterministic(dev):
    from makani_amd import ops
    prd, tar, clim, wrow = _fields(dev, 2, *PROD, dtype=torch.bfloat16, seed=9)
    first = ops.geo_metric_sums(prd, tar, clim, wrow)
    for _ in range(3):
        assert torch.equal(ops.geo_metric_sums(prd, tar, clim, wrow), first)


@pytest.mark.parametrize("axis,shapes", [("h", [181, 181, 181, 178]), ("w", [180] * 8)])
def test_shard_sums_add_up(dev, axis, shapes):
    from makani_amd import ops
    from makani_amd.distributed import compute_split_shapes
    prd, tar, clim, wrow = _fields(dev, 1, *PROD, seed=11)
    full = ops.geo_metric_sums(prd, tar, clim, wrow)
    assert compute_split_shapes(PROD[1] if axis == "h" else PROD[2], len(shapes)) == shapes
    total = torch.zeros_like(full)
    o = 0
    for n in shapes:
        if axis == "h":
            part = ops.geo_metric_sums(prd[:, :, o:o + n].contiguous(), tar[:, :, o:o + n].contiguous(),
                                       clim[:, o:o + n].contiguous(), wrow[o:o + n].contiguous())
        else:
            part = ops.geo_metric_sums(prd[..., o:o + n].contiguous(), tar[..., o:o + n].contiguous(),
                                       clim[..., o:o + n].contiguous(), wrow)
        total += part
        o += n
    assert _rel_each(total, full) < 1e-6


def test_metric_classes_on_the_kernel(dev):
    from makani_amd.metrics import GeometricACC, GeometricL1, GeometricRMSE
    prd, tar, clim, _ = _fields(dev, 2, 5, 33, 64, seed=4)
    for cls in (GeometricL1, GeometricRMSE, GeometricACC):
        kw = dict(img_shape=(35, 64), crop_shape=(33, 64), crop_offset=(1, 0), normalize=True, channel_reduction="none",
                  batch_reduction="sum")
        m_dev, m_cpu = cls("legendre-gauss", **kw).to(dev), cls("legendre-gauss", **kw)
        x, y = prd - clim, tar - clim
        got = m_dev(x, y)
        want = m_cpu(x.cpu().double(), y.cpu().double())
        assert rel(got.cpu(), want) < 1e-6, cls.__name__


def test_captured_rollout_matches_eager_bitwise(dev):
    from makani_amd.metric import MetricsHandler
    C, H, W = PROD
    names = ["u10m", "t2m", "z500"] + [f"c{i}" for i in range(C - 3)]
    params = make_params(H, W, steps=2)
    params.channel_names, params.N_out_channels = names, C
    g = torch.Generator(device=dev).manual_seed(21)
    clim = 0.5 * torch.randn(C, H, W, device=dev, generator=g)
    tars = [clim + torch.randn(1, C, H, W, device=dev, generator=g) for _ in range(3)]
    preds = [(0.8 * t + 0.3 * torch.randn(1, C, H, W, device=dev, generator=g)).to(torch.bfloat16) for t in tars]
    losses = [torch.rand((), device=dev, generator=g) for _ in range(3)]
    h = MetricsHandler(params, 1.0 + torch.rand(C), clim, dev)
    h.initialize_buffers()

    def rollout():
        for idt in range(3):
            h.update(preds[idt], tars[idt], losses[idt], idt)

    def buffers():
        return [b.clone() for b in (h.valid_buffer, h.acc_curve, h.rmse_curve, h.acc_counter)]

    with torch.inference_mode():
        h.zero_buffers()
        rollout()
        eager = buffers()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                  # warm-up off the capture stream
            h.zero_buffers()
            rollout()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rollout()
        for _ in range(2):
            h.zero_buffers()
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(buffers(), eager):
                assert torch.equal(a, b)
    assert float(eager[3].sum()) == 3.0 and float(eager[0][2]) == 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_metrics_handler_end_to_end(dev, dtype):
    params = make_params(48, 96, (45, 90), (2, 3), "legendre_gauss", steps=3)
    clim, mult, batches = make_rollout(2, len(CHANNELS), 45, 90, 3, seed=31, n_batches=2, dtype=dtype)
    h, logs, acc, rmse = run_handler(params, mult, clim, batches, device=dev)
    assert acc.is_cuda and rmse.is_cuda
    check_handler(params, mult, clim, batches, logs, acc, rmse)
