"""world_size 2 / 4 gloo tests (CPU) of the N > 1 path: process groups, the packed all-to-all
transposes, the distributed SHT choreography, DistributedInstanceNorm2d and the shared-weight
gradient reduction -- modelled on the reference's tests/distributed/tests_fft.py (split the
global tensors, run distributed, gather, compare forward output and input gradient).

The local compute stages are HIP kernels and cannot run here, so -- in THIS TEST ONLY -- the
``makani_amd.ops`` entry points are replaced by torch-CPU stand-ins of the same contracts
(private layouts in, private layouts out); what is under test is everything around them:
which rank holds what, and that the data movement and its backward are exact.
"""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

TOL = 1e-6  # tests_fft.py:170-328 pins 1e-6 for forward output and input gradient


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ------------------------------------------------------------------ torch-CPU stand-ins (test only)
def _install_cpu_ops():
    from makani_amd import ops

    # kmajor: the latitude-major layout [K, M, BC] of the Fourier rows (distributed.py), else [M, K, BC]
    def rfft(x, tw, mmax, kmajor=False):
        y = 2.0 * math.pi * torch.fft.rfft(x.float(), dim=-1, norm="forward")[..., :mmax]      # [BC, K, M]
        return (y.permute(1, 2, 0) if kmajor else y.permute(2, 1, 0)).contiguous()

    def irfft(xf, tw, nlon, out_dtype=torch.float32, kmajor=False):
        xs = xf.permute(2, 0, 1) if kmajor else xf.permute(2, 1, 0)                             # [BC, K, M]
        return torch.fft.irfft(xs, n=nlon, dim=-1, norm="forward").contiguous().to(out_dtype)

    def legendre_fwd(xf, table, lmax, m_off=0, kmajor=False):
        if kmajor:
            xf = xf.permute(1, 0, 2)
        mloc, k, _ = xf.shape
        t = table[m_off:m_off + mloc, :, :k].to(xf.dtype)
        return torch.einsum("mlk,mkn->lmn", t, xf).contiguous()

    def legendre_inv(c, table, nlat, m_off=0, kmajor=False):
        mloc = c.shape[1]
        t = table[m_off:m_off + mloc, :, :nlat].to(c.dtype)
        return torch.einsum("mlk,lmn->kmn" if kmajor else "mlk,lmn->mkn", t, c).contiguous()

    def rfft_pm(x, tw, mmax, chans, cpp):                                                      # [P, K, M, B * cpp]
        y = rfft(x, tw, mmax, True)
        K, M, bc = y.shape
        return y.view(K, M, bc // chans, chans // cpp, cpp).permute(3, 0, 1, 2, 4).reshape(chans // cpp, K, M, -1).contiguous()

    def irfft_pm(xf, tw, nlon, out_dtype, chans, cpp):
        P, K, M, bcp = xf.shape
        y = xf.view(P, K, M, bcp // cpp, cpp).permute(1, 2, 3, 0, 4).reshape(K, M, -1).contiguous()
        return irfft(y, tw, nlon, out_dtype, True)

    ops.fft_pm_supported = lambda nlon, mmax, chans, cpp: cpp > 0 and chans % cpp == 0 and cpp % 24 == 0
    ops.rfft_pm, ops.irfft_pm = rfft_pm, irfft_pm

    def spec_pack(c_std, l_off=0, m_off=0):
        return c_std.permute(1, 2, 0).contiguous()

    def spec_unpack(c_prv, l_off=0, m_off=0):
        L, M, _ = c_prv.shape
        mask = (torch.arange(L)[:, None] + l_off) >= (torch.arange(M)[None, :] + m_off)
        return (c_prv * mask[:, :, None]).permute(2, 0, 1).contiguous()

    def dhconv(x, w, batch, l_off=0, m_off=0):
        L, M, bi = x.shape
        y = torch.einsum("lmbi,iol->lmbo", x.view(L, M, batch, bi // batch), w)
        return y.reshape(L, M, -1).contiguous()

    for name, fn in dict(rfft=rfft, irfft=irfft, legendre_fwd=legendre_fwd, legendre_inv=legendre_inv,
                         spec_pack=spec_pack, spec_unpack=spec_unpack, dhconv=dhconv).items():
        setattr(ops, name, fn)


def _rel(a, b):
    return (torch.linalg.norm(a - b) / torch.linalg.norm(b)).item()


def _gather(x, dim, name):
    """all-gather uneven shards along dim (test helper, like tests_fft.py's gather)."""
    from makani_amd import comm
    size = comm.get_size(name)
    if size == 1:
        return x
    sizes = [torch.zeros(1, dtype=torch.long) for _ in range(size)]
    dist.all_gather(sizes, torch.tensor([x.shape[dim]]), group=comm.get_group(name))
    sizes = [int(s) for s in sizes]
    pad = max(sizes) - x.shape[dim]
    xp = x.contiguous()
    if pad:   # gloo all_gather needs equal shapes: pad to the largest shard, trim after
        shp = list(x.shape)
        shp[dim] = pad
        xp = torch.cat([xp, torch.zeros(shp, dtype=x.dtype)], dim=dim)
    outs = [torch.empty_like(xp) for _ in range(size)]
    dist.all_gather(outs, xp, group=comm.get_group(name))
    return torch.cat([o.narrow(dim, 0, s) for o, s in zip(outs, sizes)], dim=dim)


def _shard(x, dim, name):
    from makani_amd import comm
    from makani_amd.distributed import split_tensor_along_dim
    if comm.get_size(name) == 1:
        return x
    return split_tensor_along_dim(x, dim, comm.get_size(name))[comm.get_rank(name)].contiguous()


# ------------------------------------------------------------------ per-rank bodies
def _worker(rank, world, port, hsize, wsize, what, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        torch.set_num_threads(1)
        from makani_amd import comm
        comm.init(model_parallel_sizes=[hsize, wsize, 1, 1], backend="gloo")
        _install_cpu_ops()
        globals()["_body_" + what](rank, world)
        dist.barrier()
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _body_groups(rank, world):
    from makani_amd import comm
    h, w = comm.get_size("h"), comm.get_size("w")
    assert comm.get_size("spatial") == h * w == comm.get_size("model")
    assert comm.get_size("data") == world // (h * w)
    assert comm.get_rank("h") == rank % h and comm.get_rank("w") == (rank // h) % w
    assert comm.get_size("matmul") == 1 and comm.get_group("fin") is None
    # every rank of the h group sees the same w coordinate
    t = torch.tensor([float(comm.get_rank("w"))])
    if h > 1:
        dist.all_reduce(t, group=comm.get_group("h"))
        assert t.item() == h * comm.get_rank("w")


def _body_transpose(rank, world):
    from makani_amd import comm
    from makani_amd.distributed import distributed_transpose_polar, compute_split_shapes
    torch.manual_seed(333)
    h = comm.get_size("h")
    full = torch.complex(torch.randn(5, 7, 2, 6), torch.randn(5, 7, 2, 6))   # [M, K, B, C]
    lat_shapes = compute_split_shapes(7, h)
    x = _shard(full, 1, "h").clone().requires_grad_(True)                  # lat-sharded, all channels
    y = distributed_transpose_polar.apply(x, (3, 1), lat_shapes)            # channel-sharded, all lats
    assert torch.equal(y, _shard(full, 3, "h"))
    g = torch.complex(torch.randn(5, 7, 2, 6), torch.randn(5, 7, 2, 6))
    y.backward(_shard(g, 3, "h"))
    assert torch.equal(x.grad, _shard(g, 1, "h"))
    # and back
    z = distributed_transpose_polar.apply(y.detach(), (1, 3), compute_split_shapes(6, h))
    assert torch.equal(z, x.detach())


def _body_sht(rank, world):
    from makani_amd import comm
    from makani_amd.distributed import DistributedRealSHT, DistributedInverseRealSHT
    from oracle import spectral as osp
    torch.manual_seed(333)
    # C = 6: generic transposes; C = 48 with h = 2: channel blocks of 24 -> the peer-major (copy-free) latitude exchange
    for grid, (nlat, nlon, lmax, mmax, B, C) in (("equiangular", (33, 64, 16, 17, 2, 6)), ("legendre-gauss", (33, 64, 16, 17, 2, 6)),
                                                 ("equiangular", (33, 64, 16, 17, 2, 48))):
        f = DistributedRealSHT(nlat, nlon, lmax, mmax, grid)
        fi = DistributedInverseRealSHT(nlat, nlon, lmax, mmax, grid)
        assert f.lat_shapes == [17, 16][: comm.get_size("h")] or comm.get_size("h") == 1
        fo, fio = osp.TorchRealSHT(nlat, nlon, lmax, mmax, grid), osp.TorchInverseRealSHT(nlat, nlon, lmax, mmax, grid)
        xg = torch.randn(B, C, nlat, nlon)
        gg = torch.complex(torch.randn(B, C, lmax, mmax), torch.randn(B, C, lmax, mmax))
        # serial oracle
        xo = xg.clone().requires_grad_(True)
        co = fo(xo)
        co.backward(gg)
        # distributed
        xl = _shard(_shard(xg, 2, "h"), 3, "w").clone().requires_grad_(True)
        cl = f(xl)
        assert cl.shape == (B, C, f.l_shapes[comm.get_rank("h")], f.m_shapes[comm.get_rank("w")])
        cl.backward(_shard(_shard(gg, 2, "h"), 3, "w"))
        cfull = _gather(_gather(cl.detach(), 2, "h"), 3, "w")
        gfull = _gather(_gather(xl.grad, 2, "h"), 3, "w")
        assert _rel(cfull, co.detach()) < TOL and _rel(gfull, xo.grad) < TOL
        # inverse
        cg = co.detach().clone().requires_grad_(True)
        yo = fio(cg)
        gy = torch.randn_like(yo)
        yo.backward(gy)
        clx = _shard(_shard(co.detach(), 2, "h"), 3, "w").clone().requires_grad_(True)
        yl = fi(clx)
        assert yl.shape == (B, C, fi.lat_shapes[comm.get_rank("h")], fi.lon_shapes[comm.get_rank("w")])
        yl.backward(_shard(_shard(gy, 2, "h"), 3, "w"))
        yfull = _gather(_gather(yl.detach(), 2, "h"), 3, "w")
        gcfull = _gather(_gather(clx.grad, 2, "h"), 3, "w")
        assert _rel(yfull, yo.detach()) < TOL
        mask = (torch.arange(lmax)[:, None] >= torch.arange(mmax)[None, :])
        assert _rel(gcfull * mask, cg.grad * mask) < TOL


def _body_norm(rank, world):
    from makani_amd.layer_norm import DistributedInstanceNorm2d
    torch.manual_seed(333)
    B, C, H, W = 3, 4, 9, 10   # uneven latitude shards, batch > 1 (reference reshape bug fixed)
    xg = torch.randn(B, C, H, W) * 2 + 1
    ref = torch.nn.InstanceNorm2d(C, eps=1e-6, affine=True)
    with torch.no_grad():
        ref.weight.normal_()
        ref.bias.normal_()
    nrm = DistributedInstanceNorm2d(C, eps=1e-6, affine=True)
    nrm.load_state_dict(ref.state_dict())
    xo = xg.clone().requires_grad_(True)
    yo = ref(xo)
    gy = torch.randn_like(yo)
    yo.backward(gy)
    xl = _shard(_shard(xg, 2, "h"), 3, "w").clone().requires_grad_(True)
    yl = nrm(xl)
    yl.backward(_shard(_shard(gy, 2, "h"), 3, "w"))
    assert _rel(_gather(_gather(yl.detach(), 2, "h"), 3, "w"), yo.detach()) < 1e-5
    assert _rel(_gather(_gather(xl.grad, 2, "h"), 3, "w"), xo.grad) < 1e-5
    from makani_amd import mappings
    mappings.reduce_shared_gradients(nrm)    # weight/bias are shared over "spatial": SUM of partial grads
    assert _rel(nrm.weight.grad, ref.weight.grad) < 1e-5 and _rel(nrm.bias.grad, ref.bias.grad) < 1e-5


def _body_net(rank, world):
    from makani_amd import comm, mappings
    from makani_amd.sfnonet import SphericalFourierNeuralOperatorNet
    from makani_amd.distributed import compute_split_shapes
    from oracle import spectral as osp
    torch.manual_seed(333)
    kw = dict(inp_shape=(33, 64), out_shape=(33, 64), scale_factor=2, inp_chans=4, out_chans=3, embed_dim=6, num_layers=2)
    ref = osp.SphericalFourierNeuralOperatorNet(**kw)
    net = SphericalFourierNeuralOperatorNet(**kw)
    hs, hr = comm.get_size("h"), comm.get_rank("h")
    sd = ref.state_dict()
    for k in list(sd):
        if k.endswith("filter.filter.weight"):   # dhconv weights are sharded along l over h (spectral_convolution.py:104-107)
            lsh = compute_split_shapes(sd[k].shape[-1], hs)
            sd[k] = torch.split(sd[k], lsh, dim=-1)[hr].contiguous()
    net.load_state_dict(sd, strict=True)
    B = 2
    xg, tg = torch.randn(B, 4, 33, 64), torch.randn(B, 3, 33, 64)
    xo = xg.clone().requires_grad_(True)
    yo = ref(xo)
    ((yo - tg) ** 2).sum().backward()
    xl = _shard(_shard(xg, 2, "h"), 3, "w").clone().requires_grad_(True)
    yl = net(xl)
    ((yl - _shard(_shard(tg, 2, "h"), 3, "w")) ** 2).sum().backward()
    mappings.reduce_shared_gradients(net)
    assert _rel(_gather(_gather(yl.detach(), 2, "h"), 3, "w"), yo.detach()) < 2e-5
    assert _rel(_gather(_gather(xl.grad, 2, "h"), 3, "w"), xo.grad) < 2e-5
    po = dict(ref.named_parameters())
    scale = float(np.median([p.grad.norm().item() for p in po.values()]))
    for n, p in net.named_parameters():
        want = po[n].grad
        if n.endswith("filter.filter.weight"):
            want = torch.split(want, compute_split_shapes(want.shape[-1], hs), dim=-1)[hr]
        err = (torch.linalg.norm(p.grad - want) / max(torch.linalg.norm(want).item(), 0.1 * scale)).item()
        assert err < 5e-5, (n, err)


def _body_loss(rank, world):
    """LossHandler under spatial parallelism (losses.py:149-157): shards in, the global loss and exact shard gradients out."""
    from types import SimpleNamespace
    from makani_amd.losses import LossHandler
    from oracle import losses as ol
    H, W, C = 33, 64, 3
    params = SimpleNamespace(loss="absolute squared geometric l2", n_future=0, img_shape_x=H, img_shape_y=W, img_crop_shape_x=H,
                             img_crop_shape_y=W, img_crop_offset_x=0, img_crop_offset_y=0, N_out_channels=C,
                             channel_names=["a", "b", "c"], channel_weights="auto", model_grid_type="equiangular")
    g = torch.Generator().manual_seed(8)
    prd, tar = torch.randn(2, C, H, W, generator=g), torch.randn(2, C, H, W, generator=g)
    handler = LossHandler(params)
    handler.train()
    pl = _shard(_shard(prd, 2, "h"), 3, "w").clone().requires_grad_(True)
    loss = handler(pl, _shard(_shard(tar, 2, "h"), 3, "w"), None)
    loss.backward()
    q = ol.quad_weight("naive", (H, W), (H, W), (0, 0), normalize=True)
    want = ol.geometric_lp_loss(prd.numpy(), tar.numpy(), np.full((1, C), 1.0 / C), q, p=2, absolute=True, squared=True)
    assert abs(float(loss) - want) < 2e-6 * abs(want)
    gfull = 2.0 * (prd - tar).double() * torch.from_numpy(q) / C
    assert _rel(pl.grad, _shard(_shard(gfull.float(), 2, "h"), 3, "w")) < 1e-6


def _body_ckpt(rank, world):
    """Flexible checkpoint (trainer.py:971-1098): written under this layout, it holds full-size tensors equal to the
    un-sharded model's, and loads back into the sharded model bit for bit."""
    import tempfile
    from makani_amd import checkpoint, comm
    from makani_amd.sfnonet import SphericalFourierNeuralOperatorNet
    from makani_amd.distributed import compute_split_shapes
    from oracle import spectral as osp
    torch.manual_seed(99)
    kw = dict(inp_shape=(33, 64), out_shape=(33, 64), scale_factor=2, inp_chans=4, out_chans=3, embed_dim=6, num_layers=2,
              pos_embed="direct")
    ref = osp.SphericalFourierNeuralOperatorNet(**kw)
    net = SphericalFourierNeuralOperatorNet(**kw)
    full = dict(ref.named_parameters())
    with torch.no_grad():                                      # the sharded model holds this rank's pieces of `ref`
        for k, v in net.named_parameters():
            w = full[k].detach()
            for d, group in enumerate(getattr(v, "sharded_dims_mp", [])):
                if group is not None and comm.get_size(group) > 1:
                    w = torch.split(w, compute_split_shapes(w.shape[d], comm.get_size(group)), dim=d)[comm.get_rank(group)]
            v.copy_(w)
    path = os.path.join(tempfile.gettempdir(), f"mk_flex_{os.environ['MASTER_PORT']}_mp{{mp_rank}}.tar")
    checkpoint.save_flexible_checkpoint(path, net, iters=7, epoch=3)
    dist.barrier()
    stored = torch.load(path.format(mp_rank=0), map_location="cpu", weights_only=False)
    assert stored["iters"] == 7 and stored["epoch"] == 3 and list(stored["model_state"]) == [k for k, _ in net.named_parameters()]
    for k, w in stored["model_state"].items():
        assert w.shape == full[k].shape and torch.equal(w, full[k].detach()), k
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    with torch.no_grad():
        for v in net.parameters():
            v.zero_()
    assert checkpoint.restore_flexible_checkpoint(path, net) == (7, 3)
    for k, v in net.named_parameters():
        assert torch.equal(v.detach(), before[k]), k
    with pytest.raises(NotImplementedError):
        checkpoint.restore_flexible_checkpoint(path, net, load_optimizer=True)
    dist.barrier()
    # a file whose ``params`` entry holds a pickled class (the reference stores its YParams object there) is refused by the
    # default loader (weights_only) and read only when the caller vouches for it
    import argparse
    import pickle
    path2 = path.replace("mk_flex_", "mk_flex2_")
    if rank == 0:
        stored["params"] = argparse.Namespace(nettype="sfno")
        torch.save(stored, path2.format(mp_rank=0))
    dist.barrier()
    with pytest.raises(pickle.UnpicklingError):
        checkpoint.restore_flexible_checkpoint(path2, net)
    assert checkpoint.restore_flexible_checkpoint(path2, net, trusted_pickle=True) == (7, 3)
    dist.barrier()
    if rank == 0:
        os.remove(path.format(mp_rank=0))
        os.remove(path2.format(mp_rank=0))


def _body_fft2(rank, world):
    """The reference's own distributed test (tests/distributed/tests_fft.py:170-328, the 2-D cases): split the global
    tensors, run the distributed transform, gather, compare output and input gradient with the local transform at 1e-6."""
    from makani_amd import comm
    from makani_amd.distributed import DistributedInverseRealFFT2, DistributedRealFFT2
    from makani_amd.layers import InverseRealFFT2, RealFFT2
    torch.manual_seed(333)

    def err(a, b):
        return torch.mean(torch.norm(a - b, p=2, dim=(-1, -2)) / torch.norm(b, p=2, dim=(-1, -2))).item()

    for nlat, nlon, B, C in ((256, 512, 4, 8), (361, 720, 1, 10)):       # tests_fft.py:170-175 (batch 32 -> 4: CPU time)
        fwd_l, fwd_d = RealFFT2(nlat, nlon), DistributedRealFFT2(nlat, nlon)
        inp = torch.randn(B, C, nlat, nlon).requires_grad_(True)
        out = fwd_l(inp)
        og = torch.randn_like(out)
        out.backward(og)
        inp_l = _shard(_shard(inp.detach(), 3, "w"), 2, "h").clone().requires_grad_(True)
        out_l = fwd_d(inp_l)
        out_l.backward(_shard(_shard(og, 3, "w"), 2, "h"))
        assert tuple(out_l.shape[-2:]) == (fwd_d.l_shapes[comm.get_rank("h")], fwd_d.m_shapes[comm.get_rank("w")])
        assert err(_gather(_gather(out_l.detach(), 3, "w"), 2, "h"), out.detach()) <= TOL
        assert err(_gather(_gather(inp_l.grad, 3, "w"), 2, "h"), inp.grad) <= TOL
        # inverse (tests_fft.py:245-328)
        inv_l, inv_d = InverseRealFFT2(nlat, nlon), DistributedInverseRealFFT2(nlat, nlon)
        spec = fwd_l(torch.randn(B, C, nlat, nlon)).detach().requires_grad_(True)
        back = inv_l(spec)
        bg = torch.randn_like(back)
        back.backward(bg)
        spec_l = _shard(_shard(spec.detach(), 3, "w"), 2, "h").clone().requires_grad_(True)
        back_l = inv_d(spec_l)
        back_l.backward(_shard(_shard(bg, 3, "w"), 2, "h"))
        assert err(_gather(_gather(back_l.detach(), 3, "w"), 2, "h"), back.detach()) <= TOL
        assert err(_gather(_gather(spec_l.grad, 3, "w"), 2, "h"), spec.grad) <= TOL
    # mode truncation (lmax < nlat): the zero padding between high and low latitude modes
    fwd_l, fwd_d = RealFFT2(64, 96, lmax=21, mmax=17), DistributedRealFFT2(64, 96, lmax=21, mmax=17)
    inv_l, inv_d = InverseRealFFT2(64, 96, lmax=21, mmax=17), DistributedInverseRealFFT2(64, 96, lmax=21, mmax=17)
    x = torch.randn(2, 6, 64, 96)
    y = fwd_l(x)
    yl = fwd_d(_shard(_shard(x, 3, "w"), 2, "h"))
    assert err(_gather(_gather(yl, 3, "w"), 2, "h"), y) <= TOL
    assert err(_gather(_gather(inv_d(yl), 3, "w"), 2, "h"), inv_l(y)) <= TOL


def _body_fno(rank, world):
    """The planar (FNO) variant of the network under spatial parallelism: builds on the distributed FFT pair, steps once,
    and agrees across layouts -- the gathered output of this layout equals the gathered output under any other one, checked
    through a checksum every rank computes from identically seeded weights and inputs."""
    from makani_amd import comm, mappings
    from makani_amd.sfnonet import FourierNeuralOperatorNet
    torch.manual_seed(5)
    net = FourierNeuralOperatorNet(inp_shape=(32, 48), out_shape=(32, 48), scale_factor=1, inp_chans=3, out_chans=2, embed_dim=4,
                                   num_layers=2, big_skip=True)
    x = torch.randn(2, 3, 32, 48)
    xl = _shard(_shard(x, 2, "h"), 3, "w").clone().requires_grad_(True)
    y = net(xl)
    assert tuple(y.shape) == (2, 2, net.out_shape_loc[0], net.out_shape_loc[1])
    y.square().sum().backward()
    mappings.reduce_shared_gradients(net)
    assert torch.isfinite(xl.grad).all() and all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    full = _gather(_gather(y.detach(), 2, "h"), 3, "w")
    assert tuple(full.shape) == (2, 2, 32, 48)


def _body_ddp(rank, world):
    """The reference's wrapper (mpu/mappings.py:30-174 semantics): DistributedDataParallel(find_unused_parameters=False)
    with the gradient-reduction hook, two optimizer steps; the reduced gradients equal reduce_shared_gradients' ones."""
    import copy
    from makani_amd import comm, mappings
    from makani_amd.sfnonet import SphericalFourierNeuralOperatorNet
    torch.manual_seed(333)
    kw = dict(inp_shape=(17, 32), out_shape=(17, 32), scale_factor=2, inp_chans=3, out_chans=2, embed_dim=6, num_layers=2)
    net = SphericalFourierNeuralOperatorNet(**kw)
    mappings.sync_params(net)
    twin = copy.deepcopy(net)
    for (n, p), (_, q) in zip(net.named_parameters(), twin.named_parameters()):   # deepcopy drops the annotations
        for a in ("is_shared_mp", "sharded_dims_mp"):
            if hasattr(p, a):
                setattr(q, a, getattr(p, a))
    ddp = mappings.init_gradient_reduction_hooks(net, device_ids=None, output_device=None, find_unused_parameters=False)
    opt = torch.optim.SGD(ddp.parameters(), lr=1e-2)
    lat = net.inp_shape_loc[0]
    torch.manual_seed(1000 + comm.get_rank("data"))          # different samples per data rank
    for step in range(2):                                       # step 2 raises if a parameter got no gradient in step 1
        x, t = torch.randn(2, 3, lat, 32), torch.randn(2, 2, lat, 32)
        opt.zero_grad(set_to_none=True)
        ((ddp(x) - t) ** 2).sum().backward()
        if step == 0:
            twin.zero_grad(set_to_none=True)
            ((twin(x) - t) ** 2).sum().backward()
            mappings.reduce_shared_gradients(twin)
            for (n, p), (_, q) in zip(net.named_parameters(), twin.named_parameters()):
                assert p.grad is not None, n
                assert _rel(torch.view_as_real(p.grad) if p.grad.is_complex() else p.grad,
                            torch.view_as_real(q.grad) if q.grad.is_complex() else q.grad) < 1e-6 or q.grad.abs().max() < 1e-12, n
        opt.step()


def _body_sht721(rank, world):
    """BASELINE.json configs[3] / [4] shard shapes on the production grid: 721 latitudes over h = 4 -> [181, 181, 181,
    178], over h = 8 -> [91] * 7 + [84]; 240 degrees evenly; analysis + synthesis against the serial oracle."""
    from makani_amd import comm
    from makani_amd.distributed import DistributedRealSHT, DistributedInverseRealSHT, compute_split_shapes
    from oracle import spectral as osp
    torch.manual_seed(333)
    h = comm.get_size("h")
    nlat, nlon, lmax, mmax, B, C = 721, 1440, 240, 241, 1, h
    f = DistributedRealSHT(nlat, nlon, lmax, mmax, "equiangular")
    fi = DistributedInverseRealSHT(nlat, nlon, lmax, mmax, "equiangular")
    want = {4: [181, 181, 181, 178], 8: [91] * 7 + [84]}[h]
    assert f.lat_shapes == want and fi.lat_shapes == want and f.l_shapes == [lmax // h] * h
    assert compute_split_shapes(C, h) == [1] * h
    fo, fio = osp.TorchRealSHT(nlat, nlon, lmax, mmax, "equiangular"), osp.TorchInverseRealSHT(nlat, nlon, lmax, mmax, "equiangular")
    xg = torch.randn(B, C, nlat, nlon)
    co = fo(xg)
    cl = f(_shard(xg, 2, "h"))
    assert cl.shape == (B, C, lmax // h, mmax)
    assert _rel(_gather(cl, 2, "h"), co) < TOL
    yl = fi(_shard(co, 2, "h"))
    assert yl.shape == (B, C, want[comm.get_rank("h")], nlon)
    assert _rel(_gather(yl, 2, "h"), fio(co)) < TOL


# ------------------------------------------------------------------ launcher
def _run(world, hsize, wsize, what):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, hsize, wsize, what, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    bad = [r for r in results if r[1] != "ok"]
    assert not bad, "\n".join(f"rank {r}: {m}" for r, m in bad)


@pytest.mark.parametrize("what", ["groups", "transpose", "sht", "norm", "net"])
def test_h2(what):
    _run(2, 2, 1, what)


@pytest.mark.parametrize("what", ["groups", "sht", "net"])
def test_h2_w2(what):
    _run(4, 2, 2, what)


def test_loss_handler_gathers_spatial_shards():
    _run(4, 2, 2, "loss")


@pytest.mark.parametrize("hsize,wsize", [(2, 1), (2, 2)])
def test_flexible_checkpoint(hsize, wsize):
    _run(hsize * wsize, hsize, wsize, "ckpt")


@pytest.mark.parametrize("hsize,wsize", [(2, 1), (1, 2), (2, 2)])
def test_distributed_planar_fft_like_the_reference(hsize, wsize):
    _run(hsize * wsize, hsize, wsize, "fft2")


def test_fno_variant_under_spatial_parallelism():
    _run(2, 2, 1, "fno")


def test_data_parallel_times_h():
    _run(4, 2, 1, "groups")


def test_ddp_wrapper_data_parallel():
    _run(2, 1, 1, "ddp")


def test_ddp_wrapper_model_parallel():
    _run(2, 2, 1, "ddp")


@pytest.mark.parametrize("h", [4, 8])
def test_production_grid_shards(h):
    _run(h, h, 1, "sht721")


@pytest.mark.parametrize("ranks", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("size", [1, 5, 33, 60, 721])
def test_shard_span_is_this_ranks_entry_of_the_split_shapes(size, ranks, monkeypatch):
    """``shard_span`` for every rank of an axis, the comm sizes and ranks patched: the offset is the sum of the earlier
    ``compute_split_shapes`` entries, the length this rank's entry, and the parts tile the axis.  The other axis has one rank
    and gives ``(0, size)``."""
    from makani_amd import comm
    from makani_amd.distributed import compute_split_shapes, shard_span
    shapes = compute_split_shapes(size, ranks)
    assert len(shapes) == ranks and sum(shapes) == size
    for axis, other in (("h", "w"), ("w", "h")):
        end = 0
        for rank in range(ranks):
            monkeypatch.setattr(comm, "get_size", lambda name: ranks if name == axis else 1)
            monkeypatch.setattr(comm, "get_rank", lambda name: rank if name == axis else 0)
            off, length = shard_span(size, axis)
            assert (off, length) == (sum(shapes[:rank]), shapes[rank]) and off == end
            assert shard_span(size, other) == (0, size)
            end = off + length
        assert end == size
