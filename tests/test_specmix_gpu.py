"""The spectral channel mix (``mk_spec_mix_*``) and the two call sites that move a bias-free 1x1 convolution across a
spherical harmonic transform (the encoder's last convolution into block 0's spectrum, the last block's outer skip into the
spectrum its residual is synthesised from): kernels against float64 einsums, the streaming kernels of the new block tail
against their float64 composition, the net with ``MK_SPEC_MIX=1`` against ``MK_SPEC_MIX=0``, two latitude shards against
the serial oracle, and HIP-graph capture / replay of a step on the new path.

Tolerances.  x3 kernels: 1e-5 relative L2, the criterion of tests/test_kernels_gpu.py.  bf16 streaming kernels: one
round-to-nearest bf16 store per element bounds the relative error of an element by 2^-9, so 2^-8 = 3.9e-3 bounds the relative
L2 error with a factor two to spare; their fp32 row sums are taken before that rounding (1e-4: fp32 accumulation of 1e3..1e4
terms).  The inverse FFT with the
affine-add epilogue: the same two bounds against irfft in float64.  Net A/B under bf16 autocast: 2e-2 with the gradient floor of tests/test_model_gpu.py:250-252; in fp32 mode 1e-5.
Shards: the 8e-2 / 0.1 x median-norm floor of tests/test_distributed_gpu.py (bf16 step against the fp32 serial oracle)."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

TOL = 1e-5


def rel(a, b):
    a = np.asarray(a).astype(np.complex128 if np.iscomplexobj(a) or np.iscomplexobj(b) else np.float64)
    b = np.asarray(b)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _f64(t):
    t = t.detach().cpu()
    return t.to(torch.complex128) if t.is_complex() else t.double()


def trel(a, b, floor=0.0):
    a, b = _f64(a), _f64(b)
    return (torch.linalg.norm(a - b) / max(torch.linalg.norm(b).item(), floor)).item()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from makani_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


MIX_CASES = [
    (240, 241, 1, 384, 384, 0, 0),      # production: the benchmark's spectrum, 384 -> 384
    (16, 17, 2, 32, 32, 0, 0),          # small, ragged rows
    (12, 9, 2, 34, 38, 7, 5),           # a shard: non-zero l_off / m_off, channel counts that are even but not multiples of 4
    (9, 40, 3, 136, 70, 30, 0),         # > 64 rows (m, b) per degree and > 128 channels: several tiles each way
]


@pytest.mark.parametrize("L,M,B,I,O,l_off,m_off", MIX_CASES)
def test_spec_mix_fwd_dgrad_wgrad(dev, L, M, B, I, O, l_off, m_off):
    """fwd, dgrad and wgrad against float64 einsums over the valid entries (global m <= l); the inputs hold NaN at l < m, so a
    kernel that read one of them would poison its result."""
    from makani_amd import ops
    rng = np.random.default_rng(5)

    def crand(*s):
        return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)

    x, gy = crand(L, M, B, I), crand(L, M, B, O)
    w = rng.standard_normal((O, I)).astype(np.float32)
    mask = ((np.arange(L)[:, None] + l_off) >= (np.arange(M)[None, :] + m_off))[:, :, None, None]
    xm, gym = np.where(mask, x, 0).astype(np.complex128), np.where(mask, gy, 0).astype(np.complex128)
    nan = np.complex64(complex(np.nan, np.nan))
    xd = torch.from_numpy(np.where(mask, x, nan).reshape(L, M, B * I)).to(dev)
    gyd = torch.from_numpy(np.where(mask, gy, nan).reshape(L, M, B * O)).to(dev)
    wd = torch.from_numpy(w).to(dev)

    y = ops.spec_mix_fwd_raw(xd, wd, B, l_off, m_off).cpu().numpy().reshape(L, M, B, O)
    e_fwd = rel(np.where(mask, y, 0), np.einsum("oi,lmbi->lmbo", w.astype(np.float64), xm))
    gx = ops.spec_mix_dgrad_raw(gyd, wd, B, l_off, m_off).cpu().numpy().reshape(L, M, B, I)
    e_dg = rel(np.where(mask, gx, 0), np.einsum("oi,lmbo->lmbi", w.astype(np.float64), gym))
    gw = ops.spec_mix_wgrad_raw(xd, gyd, B, l_off, m_off).cpu().numpy()
    e_wg = rel(gw, np.einsum("lmbo,lmbi->oi", gym, np.conj(xm)).real)
    print(f"spec_mix L={L} M={M} B={B} {I}->{O} off=({l_off},{m_off}): fwd {e_fwd:.2e} dgrad {e_dg:.2e} wgrad {e_wg:.2e}")
    assert e_fwd < TOL and e_dg < TOL and e_wg < TOL


def test_spec_mix_autograd_is_the_convolution_moved_across_the_transform(dev):
    """sht(W x) = W sht(x): the mix of the spectrum against the spectrum of the convolved field, and its autograd node
    against torch's on the einsum."""
    from makani_amd import ops
    from makani_amd.sht import RealSHT
    torch.manual_seed(2)
    B, C, O = 2, 6, 8
    sht = RealSHT(33, 64, 16, 17, "equiangular").to(dev)
    x = torch.randn(B, C, 33, 64, device=dev)
    w = torch.randn(O, C, 1, 1, device=dev, requires_grad=True)
    c = sht.forward_packed(x.view(B * C, 33, 64)).detach().requires_grad_(True)
    y = ops.spec_mix(c, w, B)
    want = sht.forward_packed(torch.einsum("oi,bihw->bohw", w.detach().view(O, C), x).reshape(B * O, 33, 64))
    tri = (torch.arange(16, device=dev)[:, None] >= torch.arange(17, device=dev)[None, :])[:, :, None]
    assert trel(torch.view_as_real(torch.where(tri, y.detach(), 0)), torch.view_as_real(torch.where(tri, want, 0))) < TOL
    g = torch.where(tri, torch.randn_like(y), 0)
    y.backward(g)
    c2 = torch.where(tri, c.detach(), 0).to(torch.complex128).view(16, 17, B, C).requires_grad_(True)
    w2 = w.detach().double().view(O, C).requires_grad_(True)
    y2 = torch.einsum("oi,lmbi->lmbo", w2.to(torch.complex128), c2)
    y2.backward(g.to(torch.complex128).view(16, 17, B, O))
    assert trel(torch.view_as_real(torch.where(tri, c.grad, 0)), torch.view_as_real(c2.grad.reshape(16, 17, B * C))) < TOL
    assert trel(w.grad.view(O, C), w2.grad) < TOL


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_affine_add_and_gelu_backward_vs_float64(dev, dtype):
    """The two streaming kernels of the new path: y = r + a z + b per row, and gpre = g gelu'(pre) with its row sums."""
    from makani_amd import ops
    torch.manual_seed(11)
    B, C, H, W = 2, 5, 12, 42            # H * W = 504: a multiple of 8 with a ragged last vector step
    r, z = torch.randn(B, C, H, W, device=dev).to(dtype), torch.randn(B, C, H, W, device=dev).to(dtype)
    aff = torch.randn(B * C, 2, device=dev)
    tol = 1e-6 if dtype == torch.float32 else 2.0 ** -8
    y = ops.affine_add(r, z, aff)
    want = r.double() + aff[:, 0].double().view(B, C, 1, 1) * z.double() + aff[:, 1].double().view(B, C, 1, 1)
    e_y = trel(y, want)
    pre, g = torch.randn(B, C, H * W, device=dev).to(dtype), torch.randn(B, C, H * W, device=dev).to(dtype)
    gp, gs = ops.gelu_backward(pre, g, True)
    p64 = pre.double()
    d = 0.5 * (1 + torch.erf(p64 / 2 ** 0.5)) + p64 * torch.exp(-0.5 * p64 * p64) / (2 * torch.pi) ** 0.5
    e_g, e_s = trel(gp, g.double() * d), trel(gs, (g.double() * d).sum((0, 2)))
    print(f"{dtype}: affine_add {e_y:.2e}, gelu_backward {e_g:.2e}, row sums {e_s:.2e}")
    assert e_y < tol and e_g < tol and e_s < (1e-6 if dtype == torch.float32 else 1e-4)
    assert ops.gelu_backward(pre, g)[1] is None


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("nlon,kmajor", [(480, True), (1440, True), (1440, False)])
def test_irfft_affine_add_vs_float64(dev, dtype, nlon, kmajor):
    """The inverse FFT with the affine-add epilogue against irfft in float64 plus a z + b (fp32 rows: the 1e-5 of the
    spectral kernels; bf16 rows: one rounding of the stored value)."""
    from makani_amd import ops
    torch.manual_seed(13)
    BC, K, M = 20, 5, 200            # 20 rows: a partial tile of 24 (nlon 480) and of 8 (nlon 1440)
    xf = torch.randn(K, M, BC, dtype=torch.complex64, device=dev) if kmajor else torch.randn(M, K, BC, dtype=torch.complex64, device=dev)
    z = torch.randn(BC, K, nlon, device=dev).to(dtype)
    aff = torch.randn(BC, 2, device=dev)
    got = ops.irfft_affine_add_raw(xf, ops.fft_twiddles(nlon).to(dev), nlon, z, aff, kmajor)
    spec = (xf.permute(2, 0, 1) if kmajor else xf.permute(2, 1, 0)).to(torch.complex128)         # [BC, K, M]
    want = torch.fft.irfft(spec, n=nlon, dim=-1, norm="forward") + aff[:, 0].double().view(BC, 1, 1) * z.double() \
        + aff[:, 1].double().view(BC, 1, 1)
    err = trel(got, want)
    print(f"irfft_affine_add nlon={nlon} kmajor={kmajor} {dtype}: {err:.2e}")
    assert got.dtype == dtype and err < (TOL if dtype == torch.float32 else 2.0 ** -8)


def test_net_irfft_affine_add_on_equals_off(dev, monkeypatch):
    """A net whose output grid has a length the split FFT kernels serve: the block tail with the add folded into the inverse
    FFT (MK_IRFFT_AFFINE_ADD=1, one such launch per forward pass) against the separate streaming pass (0)."""
    from makani_amd import ops
    from makani_amd.sfnonet import SphericalFourierNeuralOperatorNet
    torch.manual_seed(21)
    kw = dict(inp_shape=(24, 480), out_shape=(24, 480), scale_factor=2, inp_chans=6, out_chans=5, embed_dim=32, num_layers=2)
    net = SphericalFourierNeuralOperatorNet(**kw).to(dev)
    x, tar = torch.randn(2, 6, 24, 480, device=dev), torch.randn(2, 5, 24, 480, device=dev)
    calls, real = [], ops.irfft_affine_add_raw
    monkeypatch.setattr(ops, "irfft_affine_add_raw", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    res = {}
    for on in ("1", "0"):
        monkeypatch.setenv("MK_IRFFT_AFFINE_ADD", on)
        net.zero_grad(set_to_none=True)
        xd = x.clone().requires_grad_(True)
        del calls[:]
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = net(xd)
        assert len(calls) == (1 if on == "1" else 0)
        ((y.float() - tar) ** 2).mean().backward()
        grads = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
        grads["input"] = xd.grad.detach().clone()
        res[on] = (y.detach().float().clone(), grads)
    scale = float(np.median([torch.linalg.norm(_f64(g)).item() for n, g in res["0"][1].items() if n != "input"]))
    e_y = trel(res["1"][0], res["0"][0])
    errs = {n: trel(res["1"][1][n], res["0"][1][n], floor=scale) for n in res["1"][1]}
    worst = max(errs, key=errs.get)
    print(f"irfft affine add on/off: output {e_y:.2e}, worst gradient {worst} {errs[worst]:.2e}")
    assert e_y < 2e-2 and errs[worst] < 2e-2, (worst, errs[worst])


NET_KW = dict(inp_shape=(32, 64), out_shape=(32, 64), scale_factor=2, inp_chans=6, out_chans=5, embed_dim=32, num_layers=2)


def _count_mix_calls(monkeypatch):
    from makani_amd import ops
    calls, real = [], ops.spec_mix
    monkeypatch.setattr(ops, "spec_mix", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("amp", [False, True])
def test_net_spec_mix_on_equals_off(dev, monkeypatch, amp):
    """A resolution-changing two-block net with MK_SPEC_MIX=1 against 0: output, every parameter gradient and the input
    gradient.  Under bf16 autocast both convolutions move (two mix launches per forward pass); the fp32 mode keeps the
    convolutions on the grid either way."""
    from makani_amd.sfnonet import SphericalFourierNeuralOperatorNet
    torch.manual_seed(9)
    net = SphericalFourierNeuralOperatorNet(**NET_KW).to(dev)
    x, tar = torch.randn(2, 6, 32, 64, device=dev), torch.randn(2, 5, 32, 64, device=dev)
    calls = _count_mix_calls(monkeypatch)
    res = {}
    for on in ("1", "0"):
        monkeypatch.setenv("MK_SPEC_MIX", on)
        net.zero_grad(set_to_none=True)
        xd = x.clone().requires_grad_(True)
        del calls[:]
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            y = net(xd)
        assert len(calls) == (2 if (amp and on == "1") else 0)
        ((y.float() - tar) ** 2).mean().backward()
        grads = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
        grads["input"] = xd.grad.detach().clone()
        res[on] = (y.detach().float().clone(), grads)
    tol = 2e-2 if amp else 1e-5
    scale = float(np.median([torch.linalg.norm(_f64(g)).item() for n, g in res["0"][1].items() if n != "input"]))
    e_y = trel(res["1"][0], res["0"][0])
    errs = {n: trel(res["1"][1][n], res["0"][1][n], floor=scale if amp else 0.0) for n in res["1"][1]}
    worst = max(errs, key=errs.get)
    print(f"amp={amp}: output {e_y:.2e}, worst gradient {worst} {errs[worst]:.2e}")
    assert e_y < tol
    assert errs[worst] < tol, (worst, errs[worst])


def test_net_spec_mix_vs_oracle_bf16(dev):
    """The new path against the fp32 CPU oracle at the bf16 accuracy the engine path is held to (tests/test_model_gpu.py)."""
    from makani_amd.sfnonet import SphericalFourierNeuralOperatorNet
    from oracle import spectral as osp
    torch.manual_seed(9)
    ref = osp.SphericalFourierNeuralOperatorNet(**NET_KW)
    net = SphericalFourierNeuralOperatorNet(**NET_KW).to(dev)
    net.load_state_dict(ref.state_dict())
    x, tar = torch.randn(2, 6, 32, 64), torch.randn(2, 5, 32, 64)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = net(x.to(dev))
    ((y.float() - tar.to(dev)) ** 2).mean().backward()
    yo = ref(x)
    ((yo - tar) ** 2).mean().backward()
    assert trel(y.float(), yo) < 3e-2
    po = dict(ref.named_parameters())
    scale = float(np.median([torch.linalg.norm(_f64(p.grad)).item() for p in po.values()]))
    errs = {n: trel(p.grad, po[n].grad, floor=scale) for n, p in net.named_parameters()}
    worst = max(errs, key=errs.get)
    assert errs[worst] < 5e-2, (worst, errs[worst])


def test_graph_capture_replay_with_spec_mix(dev, monkeypatch):
    """Capture forward + loss + backward of a net on the new path in a HIP graph (the sequence of
    tests/test_model_gpu.py::test_hip_graph_capture_replay); replays reproduce the eager numbers."""
    import gc
    from makani_amd.sfnonet import SphericalFourierNeuralOperatorNet
    monkeypatch.setenv("MK_SPEC_MIX", "1")
    torch.manual_seed(7)
    net = SphericalFourierNeuralOperatorNet(**NET_KW).to(dev)
    x, tar = torch.randn(2, 6, 32, 64, device=dev), torch.randn(2, 5, 32, 64, device=dev)
    static_inp, static_tar = x.clone(), tar.clone()
    calls = _count_mix_calls(monkeypatch)
    capture_stream = torch.cuda.Stream()
    capture_stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(capture_stream):
        for _ in range(3):
            net.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                static_loss = ((net(static_inp).float() - static_tar) ** 2).mean()
            static_loss.backward()
        capture_stream.synchronize()
        assert len(calls) == 6
        ref_loss = static_loss.item()
        ref_grads = {n: p.grad.clone() for n, p in net.named_parameters()}
        gc.collect()
        torch.cuda.empty_cache()
        graph = torch.cuda.CUDAGraph()
        net.zero_grad(set_to_none=True)
        graph.capture_begin()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            static_loss = ((net(static_inp).float() - static_tar) ** 2).mean()
        static_loss.backward()
        graph.capture_end()
    torch.cuda.current_stream().wait_stream(capture_stream)
    for _ in range(2):
        static_inp.copy_(x)
        static_tar.copy_(tar)
        graph.replay()
    torch.cuda.synchronize()
    assert abs(static_loss.item() - ref_loss) <= 1e-6 * abs(ref_loss)
    for n, p in net.named_parameters():
        assert p.grad is not None, n
        assert torch.equal(p.grad, ref_grads[n]) or trel(p.grad, ref_grads[n]) < 1e-5, n


# ---------------------------------------------------------------------------------------------------------------------
# two latitude shards on one card (the machinery of tests/test_distributed_gpu.py: gloo wire, ranks take turns on the card)
# ---------------------------------------------------------------------------------------------------------------------
def _body_moved_weights(dev):
    """h = 2, bf16 autocast, MK_SPEC_MIX=1: the gradients of the two moved weights are now partial sums over SPECTRAL shards;
    after ``reduce_shared_gradients`` they equal the serial result."""
    from test_distributed_gpu import _gather, _rel, _shard
    from makani_amd import comm, mappings, ops
    from makani_amd.distributed import compute_split_shapes
    from makani_amd.sfnonet import SphericalFourierNeuralOperatorNet
    from oracle import spectral as osp
    os.environ["MK_SPEC_MIX"] = "1"
    torch.manual_seed(77)
    kw = dict(inp_shape=(64, 128), out_shape=(64, 128), scale_factor=2, inp_chans=4, out_chans=3, embed_dim=16, num_layers=2)
    ref = osp.SphericalFourierNeuralOperatorNet(**kw)
    net = SphericalFourierNeuralOperatorNet(**kw)
    hs, hr = comm.get_size("h"), comm.get_rank("h")
    sd = ref.state_dict()
    for k in list(sd):
        if k.endswith("filter.filter.weight"):
            sd[k] = torch.split(sd[k], compute_split_shapes(sd[k].shape[-1], hs), dim=-1)[hr].contiguous()
    net.load_state_dict(sd, strict=True)
    net = net.to(dev)
    xg, tg = torch.randn(2, 4, 64, 128), torch.randn(2, 3, 64, 128)
    yo = ref(xg)
    ((yo - tg) ** 2).sum().backward()
    xl, tl = _shard(xg, 2, "h").to(dev), _shard(tg, 2, "h").to(dev)
    calls, real = [], ops.spec_mix
    ops.spec_mix = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = net(xl)
    finally:
        ops.spec_mix = real
    assert len(calls) == 2, "the sharded step did not take the spectral path"
    ((y.float() - tl) ** 2).sum().backward()
    mappings.reduce_shared_gradients(net)
    assert _rel(_gather(y.detach().float(), 2, "h"), yo.detach()) < 3e-2
    po = dict(ref.named_parameters())
    pn = dict(net.named_parameters())
    scale = float(np.median([p.grad.norm().item() for p in po.values()]))
    for n in ("encoder.fwd.2.weight", "blocks.1.outer_skip.weight"):
        err = _rel(pn[n].grad, po[n].grad, floor=0.1 * scale)
        assert err < 8e-2, f"rank {hr}: gradient of the moved weight {n}: {err:.3e}"


def _worker(rank, world, port, q, lock):
    import torch.distributed as dist
    from test_distributed_gpu import _take_turns_on_the_card
    held = False
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
        from makani_amd import comm
        comm.init(model_parallel_sizes=[world, 1, 1, 1], backend="gloo")
        _take_turns_on_the_card(lock)
        lock.acquire()
        held = True
        _body_moved_weights(torch.device("cuda:0"))
        torch.cuda.synchronize()
        dist.barrier()
        q.put((rank, "ok"))
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


def test_h2_moved_weight_gradients():
    from test_distributed_gpu import _free_port
    assert torch.cuda.device_count() >= 1
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    lock = ctx.Lock()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, lock)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    bad = [r for r in results if r[1] != "ok"]
    assert not bad, "\n".join(f"rank {r}: {m}" for r, m in bad)
