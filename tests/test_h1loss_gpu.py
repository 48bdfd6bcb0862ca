"""GPU tests of the H1 loss on per-degree HIP sums: the two kernels of csrc/specnorm.hip against float64 numpy on packed
spectra whose empty triangle (``l_off + l < m_off + m``, never written by the Legendre kernels) holds NaN, the loss and its
gradient against the oracle, graph capture, and the sharded loss (two ranks on one card) without a gather."""
import gc
import os
import socket
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_specnorm_cpu import degree_power_numpy, packed_spectrum

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7, 3), (33, 33, 146), (17, 64, 73)]          # (L, M, BC)
OFFSETS = [(0, 0), (16, 0), (0, 5), (16, 33)]               # the last one leaves whole rows (or everything) empty


def _stored(shape, offs):
    nl, nm, bc = shape
    l = torch.arange(nl).reshape(nl, 1, 1) + offs[0]
    m = torch.arange(nm).reshape(1, nm, 1) + offs[1]
    return (l >= m).expand(nl, nm, bc)


# ---------------------------------------------------------------------------------------------------------------------
# 1. kernel value
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offs", OFFSETS, ids=lambda o: f"l{o[0]}m{o[1]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_degree_power_kernel_matches_numpy(dev, shape, offs):
    """Exact squares and at most 64 additions per sum in float64: 1e-12 relative, and nothing of the NaN triangle."""
    from makani_amd import ops
    c = packed_spectrum(*shape, *offs, seed=31)
    got = ops.degree_power(c.to(dev), *offs)
    want = degree_power_numpy(c, *offs)
    assert got.dtype == torch.float64 and tuple(got.shape) == (shape[2], shape[0])
    got = got.cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - want).max()
    print(f"degree_power {shape} {offs}: max abs error {err:.3e}, max |P| {np.abs(want).max():.3e}")
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. repeatability
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: "x".join(map(str, s)))
def test_degree_power_is_repeatable_and_slices_agree(dev, shape):
    from makani_amd import ops
    nl, nm, bc = shape
    c = packed_spectrum(*shape, seed=32).to(dev)
    full = ops.degree_power(c)
    assert torch.equal(full, ops.degree_power(c))
    l0 = nl // 2 + 1
    assert torch.equal(ops.degree_power(c[l0:].contiguous(), l0, 0), full[:, l0:])
    assert torch.equal(ops.degree_power(c[:l0].contiguous(), 0, 0), full[:, :l0])
    m0 = nm // 2 + 1
    parts = ops.degree_power(c[:, :m0].contiguous(), 0, 0) + ops.degree_power(c[:, m0:].contiguous(), 0, m0)
    err = ((parts - full).abs() / full.abs().clamp_min(1e-300)).max().item()
    print(f"m slices vs whole {shape}: {err:.3e}")
    assert err <= 1e-13


# ---------------------------------------------------------------------------------------------------------------------
# 3. backward kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offs", OFFSETS, ids=lambda o: f"l{o[0]}m{o[1]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_degree_power_backward_kernel(dev, shape, offs):
    """gc = 2 w gP c formed in float64 and rounded to fp32: equal within one fp32 ulp; exact zeros in the NaN triangle."""
    from makani_amd import ops
    nl, nm, bc = shape
    c = packed_spectrum(*shape, *offs, seed=33)
    g = torch.randn(bc, nl, dtype=torch.float64, generator=torch.Generator().manual_seed(34))
    x = c.to(dev).requires_grad_(True)
    ops.degree_power(x, *offs).backward(g.to(dev))
    got = x.grad.cpu()
    stored = _stored(shape, offs)
    assert torch.equal(torch.view_as_real(got)[~stored], torch.zeros_like(torch.view_as_real(got)[~stored]))
    m = torch.arange(nm).reshape(1, nm, 1) + offs[1]
    k = 2 * torch.where(m == 0, 1.0, 2.0).double() * g.t().reshape(nl, 1, bc)
    for part in ("real", "imag"):
        want = (k * getattr(c, part).double())[stored].float()
        have = getattr(got, part)[stored]
        ulp = torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()
        assert ((have - want).abs() <= ulp).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. loss against the oracle
# ---------------------------------------------------------------------------------------------------------------------
B, C, H, W = 2, 3, 33, 64
_ORACLE = {}


def _fields(seed=6):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)


def _oracle(absolute, squared):
    """(value by oracle.losses.geometric_h1_loss on the oracle transform's coefficients, d value / d prd by float64 autograd
    through the oracle transform); computed once per spelling."""
    key = (absolute, squared)
    if key not in _ORACLE:
        from oracle import losses as ol
        from oracle import spectral as osp
        prd, tar = _fields()
        sht = osp.TorchRealSHT(H, W, grid="equiangular")
        po, to = prd.double().requires_grad_(True), tar.double()
        cd, ct = sht(po - to), sht(to)
        want = ol.geometric_h1_loss(cd.detach().numpy(), None if absolute else ct.numpy(), squared=squared)
        lw = torch.arange(H, dtype=torch.float64)
        lw = lw * (lw + 1)

        def norms(c):
            a = c.real ** 2 + c.imag ** 2
            n2 = a[..., 0] + 2 * a[..., 1:].sum(-1)
            return n2.reshape(B, -1).sum(-1), (n2 * lw).reshape(B, -1).sum(-1)

        def combine(l2, h1):
            return 0.5 * l2 + 0.5 * h1 if squared else 0.5 * l2.sqrt() + 0.5 * h1.sqrt()

        val = combine(*norms(cd))
        if not absolute:
            val = val / combine(*norms(ct))
        val = val.sum()
        assert abs(float(val) - want) <= 1e-12 * abs(want)
        val.backward()
        _ORACLE[key] = (want, po.grad.clone())
    return _ORACLE[key]


def _graph_names(fn, seen=None):
    seen = set() if seen is None else seen
    if fn is None or fn in seen:
        return set()
    seen.add(fn)
    names = {type(fn).__name__}
    for nxt, _ in fn.next_functions:
        names |= _graph_names(nxt, seen)
    return names


@pytest.mark.parametrize("absolute", [True, False])
@pytest.mark.parametrize("squared", [True, False])
def test_h1_loss_value_and_gradient_against_the_oracle(dev, absolute, squared):
    from makani_amd.losses import GeometricH1Loss
    prd, tar = _fields()
    want, gwant = _oracle(absolute, squared)
    loss = GeometricH1Loss((H, W), absolute=absolute, squared=squared).to(dev)
    x = prd.to(dev).requires_grad_(True)
    out = loss(x, tar.to(dev))
    out.backward()
    names = _graph_names(out.grad_fn)
    assert "_DegreePowerBackward" in names and "_SpecUnpackBackward" not in names and "ViewAsRealBackward0" not in names
    assert out.dtype == torch.float32 and out.dim() == 0
    e_val = abs(float(out.detach()) - want) / abs(want)
    e_grad = (torch.linalg.norm(x.grad.cpu().double() - gwant) / torch.linalg.norm(gwant)).item()
    print(f"H1 loss absolute={absolute} squared={squared}: value {e_val:.3e}, gradient {e_grad:.3e}")
    assert e_val < 2e-5
    assert e_grad < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 5. graph capture
# ---------------------------------------------------------------------------------------------------------------------
def test_captured_h1_loss_matches_eager_bitwise(dev):
    from makani_amd.losses import GeometricH1Loss
    loss = GeometricH1Loss((H, W)).to(dev)
    inputs = [tuple(t.to(dev) for t in _fields(seed=s)) for s in (41, 42)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = []
        for p, t in inputs:
            x = p.clone().requires_grad_(True)
            out = loss(x, t)
            out.backward()
            eager.append((out.detach().clone(), x.grad.clone()))
            del out, x
        static_prd = inputs[0][0].clone().requires_grad_(True)
        static_tar = inputs[0][1].clone()
        for _ in range(2):                                             # warm-ups on the capture stream
            static_prd.grad = None
            loss(static_prd, static_tar).backward()
        static_prd.grad = None
        gc.collect()
        torch.cuda.empty_cache()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            static_out = loss(static_prd, static_tar)
            static_out.backward()
        for (p, t), (want_out, want_grad) in zip(inputs[1:] + inputs[:1], eager[1:] + eager[:1]):
            with torch.no_grad():
                static_prd.copy_(p)
                static_tar.copy_(t)
            graph.replay()
            side.synchronize()
            assert torch.equal(static_out.detach(), want_out) and torch.equal(static_prd.grad, want_grad)
    torch.cuda.current_stream().wait_stream(side)
    assert not torch.equal(eager[0][1], eager[1][1])


# ---------------------------------------------------------------------------------------------------------------------
# 6. sharded, two ranks on one card
# ---------------------------------------------------------------------------------------------------------------------
SPELLINGS = ["geometric h1", "absolute squared geometric h1"]


def _params(spec):
    return SimpleNamespace(loss=spec, n_future=0, img_shape_x=H, img_shape_y=W, img_crop_shape_x=H, img_crop_shape_y=W,
                           img_crop_offset_x=0, img_crop_offset_y=0, N_out_channels=C, channel_names=["a", "b", "c"],
                           channel_weights="auto", model_grid_type="equiangular")


class _Gathered(Exception):
    pass


def _no_gather(*args, **kwargs):
    raise _Gathered()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, along_w, q, lock):
    held = False
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK="0")
        from test_distributed_gpu import _take_turns_on_the_card
        from makani_amd import comm, losses
        from makani_amd.distributed import split_tensor_along_dim
        comm.init(model_parallel_sizes=[1, world, 1, 1] if along_w else [world, 1, 1, 1], backend="gloo")
        losses.gather_from_parallel_region = _no_gather
        dev = torch.device("cuda:0")
        _take_turns_on_the_card(lock)
        lock.acquire()
        held = True
        prd, tar = _fields()

        def shard(x):
            x = split_tensor_along_dim(x, -2, comm.get_size("h"))[comm.get_rank("h")]
            return split_tensor_along_dim(x, -1, comm.get_size("w"))[comm.get_rank("w")].contiguous()

        out = {}
        for spec in SPELLINGS:
            handler = losses.LossHandler(_params(spec)).to(dev)
            handler.train()
            assert handler.do_gather_input
            x = shard(prd).to(dev).requires_grad_(True)
            loss = handler(x, shard(tar).to(dev), None)
            loss.backward()
            out[spec] = (float(loss.detach()), x.grad.cpu())
        torch.cuda.synchronize()
        dist.barrier()
        q.put((rank, ((comm.get_rank("h"), comm.get_rank("w")), out)))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
    finally:
        if held:
            try:
                lock.release()
            except ValueError:
                pass
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("along_w", [False, True], ids=["h2", "w2"])
def test_sharded_h1_loss_equals_single_process_without_gather(dev, along_w):
    from makani_amd.distributed import compute_split_shapes
    from makani_amd.losses import LossHandler
    prd, tar = _fields()
    single = {}
    for spec in SPELLINGS:
        handler = LossHandler(_params(spec)).to(dev)
        handler.train()
        x = prd.to(dev).requires_grad_(True)
        loss = handler(x, tar.to(dev), None)
        loss.backward()
        single[spec] = (float(loss.detach()), x.grad.cpu())
    torch.cuda.synchronize()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    lock = ctx.Lock()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, along_w, q, lock)) for r in range(2)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    bad = {r: m for r, m in results.items() if isinstance(m, str)}
    assert not bad, "\n".join(f"rank {r}: {m}" for r, m in bad.items())
    hs = compute_split_shapes(H, 1 if along_w else 2)
    ws = compute_split_shapes(W, 2 if along_w else 1)
    assert sorted(w for w, _ in results.values()) == [(i, j) for i in range(len(hs)) for j in range(len(ws))]
    for r, ((i, j), out) in results.items():
        for spec in SPELLINGS:
            want, gfull = single[spec]
            got, grad = out[spec]
            gshard = gfull[:, :, sum(hs[:i]):sum(hs[:i + 1]), sum(ws[:j]):sum(ws[:j + 1])]
            e_val = abs(got - want) / abs(want)
            e_grad = (torch.linalg.norm(grad.double() - gshard.double()) / torch.linalg.norm(gshard.double())).item()
            print(f"rank {r} ({i}, {j}) '{spec}': value {e_val:.3e}, gradient {e_grad:.3e}")
            assert grad.shape == gshard.shape
            assert e_val < 1e-5 and e_grad < 1e-5, (r, spec)


# ---------------------------------------------------------------------------------------------------------------------
# the four-dimensional transform call the losses and the spectral filters share
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("grid", ["equiangular", "legendre-gauss"])
def test_forward_packed_fields_is_forward_packed_of_the_rows(dev, grid, dtype):
    """``forward_packed_fields`` of ``[2, 3, 33, 64]`` fields holds the bits of ``forward_packed`` of the ``[6, 33, 64]`` rows with
    the offsets ``(0, 0)``; a non-contiguous input gives the bits of its contiguous copy."""
    from makani_amd.sht import RealSHT
    H, W = 33, 64
    sht = RealSHT(H, W, grid=grid).to(dev)
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(5)).to(dev, dtype)
    want = sht.forward_packed(x.reshape(-1, H, W))
    got, l_off, m_off = sht.forward_packed_fields(x)
    assert (l_off, m_off) == (0, 0) and got.dtype == torch.complex64 and tuple(got.shape) == (sht.lmax, sht.mmax, 6)
    stored = _stored(tuple(got.shape), (0, 0)).to(dev)          # the Legendre kernels leave the rest unwritten
    assert torch.equal(torch.view_as_real(got)[stored], torch.view_as_real(want)[stored])
    strided = x.transpose(0, 1).contiguous().transpose(0, 1)
    assert not strided.is_contiguous() and torch.equal(strided, x)
    again = sht.forward_packed_fields(strided)[0]
    assert torch.equal(torch.view_as_real(again)[stored], torch.view_as_real(want)[stored])
