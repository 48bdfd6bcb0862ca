"""GPU tests of the multi-tensor optimizer kernels (optim.hip through makani_amd.optim): the parity cases of
test_optim_cpu.py on the kernels at production sizes, deterministic norms, capturable == eager bit for bit, and the
whole training step (forward + backward + clip + update) captured into one graph."""
import gc
import math

import pytest
import torch

from test_optim_cpu import LAMB_CASES, TOL, check_adamw, check_lamb, make_grads, make_params, rel, set_grads

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("adam_w_mode", [True, False])
@pytest.mark.parametrize("max_grad_norm", [None, 50.0])
def test_fused_adamw_kernels_match_torch(dev, adam_w_mode, max_grad_norm):
    opt, ps = check_adamw(dev, adam_w_mode, big=True, max_grad_norm=max_grad_norm)
    assert ps[2].shape == (384, 384, 240) and ps[-1].data_ptr() % 16 == 4


@pytest.mark.parametrize("case", LAMB_CASES)
def test_fused_lamb_kernels_match_apex_arithmetic(dev, case):
    check_lamb(dev, case, big=case is LAMB_CASES[1] or case is LAMB_CASES[4])
    check_lamb(dev, case, big=False)


def test_clip_grad_norm_kernels(dev):
    from makani_amd.optim import clip_grad_norm_
    ps = make_params(dev, big=True)
    gs = make_grads(ps, 1, skip=None)[0]
    norms = []
    for _ in range(3):
        set_grads(ps, gs)
        norms.append(clip_grad_norm_(ps, 1e9))
    assert all(torch.equal(n, norms[0]) for n in norms)          # bitwise deterministic
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    set_grads(ref, gs)
    set_grads(ps, gs)
    n = clip_grad_norm_(ps, 10.0)
    nr = torch.nn.utils.clip_grad_norm_(ref, 10.0)
    assert n.device.type == "cuda" and n.dim() == 0
    assert abs(n.item() - nr.item()) <= TOL * nr.item()
    for p, q in zip(ps, ref):
        assert rel(p.grad, q.grad) <= TOL


@pytest.mark.parametrize("cls", ["FusedAdamW", "FusedLAMB"])
def test_capturable_is_bitwise_the_eager_step(dev, cls):
    from makani_amd import optim
    kw = dict(lr=1e-2, weight_decay=0.1, max_grad_norm=2.0)
    runs = []
    for capturable in (False, True):
        ps = make_params(dev)
        opt = getattr(optim, cls)(ps, capturable=capturable, **kw)
        for gs in make_grads(ps, 5):
            set_grads(ps, gs)
            opt.step()
        torch.cuda.synchronize()
        runs.append((ps, opt))
    (pa, oa), (pb, ob) = runs
    for p, q in zip(pa, pb):
        assert torch.equal(p, q)
        for k in ("m", "v"):
            assert torch.equal(oa.state[p][k], ob.state[q][k])
        assert float(oa.state[p]["step"]) == float(ob.state[q]["step"])


def _synthetic(dev):
    torch.manual_seed(11)
    a = torch.nn.Parameter(torch.randn(1100, 1001, device=dev))
    b = torch.nn.Parameter(torch.randn(96, 96, 120, dtype=torch.complex64, device=dev))
    c = torch.nn.Parameter(torch.randn(1001, 1300, device=dev))
    d = torch.nn.Parameter(torch.randn(64, device=dev))
    return [a, b, c, d]


def _loss(ps, x, z):
    a, b, c, d = ps
    h = torch.tanh(x @ c[:, :1100])
    y = (h @ a) * 1e-2
    return (y ** 2).mean() + (torch.view_as_real(b * z) ** 2).mean() + (d ** 2).sum() * 1e-3


@pytest.mark.parametrize("cls", ["FusedAdamW", "FusedLAMB"])
def test_whole_step_in_one_graph_equals_eager(dev, cls):
    """forward + backward + clip_grad_norm_ + step captured into one graph: 4 replays equal 4 eager steps bit for bit,
    and a StepLR change between replays reaches the graph."""
    from makani_amd import optim
    from makani_amd.optim import clip_grad_norm_
    x = torch.randn(32, 1001, device=dev)
    z = torch.randn(96, 96, 120, dtype=torch.complex64, device=dev)

    def one_step(ps, opt):
        opt.zero_grad(set_to_none=True)
        _loss(ps, x, z).backward()
        clip_grad_norm_(ps, 1.0)
        opt.step()

    results = []
    for graphed in (False, True):
        ps = _synthetic(dev)
        opt = getattr(optim, cls)(ps, lr=1e-2, weight_decay=0.05, capturable=True)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            one_step(ps, opt)                  # warm-up (both runs)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        if graphed:
            g = torch.cuda.CUDAGraph()
            opt.zero_grad(set_to_none=True)
            with torch.cuda.graph(g):
                _loss(ps, x, z).backward()
                clip_grad_norm_(ps, 1.0)
                opt.step()
        for i in range(4):
            if i == 2:
                sched.step()
            if graphed:
                g.replay()
            else:
                one_step(ps, opt)
        torch.cuda.synchronize()
        assert abs(float(opt.param_groups[0]["lr"]) - 5e-3) < 1e-9
        results.append(([p.detach().clone() for p in ps], [opt.state[p]["m"].clone() for p in ps],
                        [float(opt.state[p]["step"]) for p in ps]))
    (pa, ma, sa), (pb, mb, sb) = results
    assert sa == sb == [5.0] * 4
    for u, v in zip(pa + ma, pb + mb):
        assert torch.equal(u, v)


def _adam_ratio_bound(b1, b2, t):
    """Largest |m^| / sqrt(v^) Adam can produce after t steps, whatever the gradients (Cauchy-Schwarz on the two
    bias-corrected weightings: (sum w_i g_i)^2 <= (sum w_i^2 / u_i) (sum u_i g_i^2))."""
    w = [(1 - b1) * b1 ** (t - i) / (1 - b1 ** t) for i in range(1, t + 1)]
    u = [(1 - b2) * b2 ** (t - i) / (1 - b2 ** t) for i in range(1, t + 1)]
    return math.sqrt(sum(wi * wi / ui for wi, ui in zip(w, u)))


def test_tiny_sfno_step_captured_with_the_optimizer(dev):
    """The tiny SFNO of test_hip_graph_capture_replay under bf16 autocast, the whole step (forward, loss, backward, clip,
    FusedAdamW) in one graph: 3 replays against 3 eager steps from the SAME state (2 shared warm-ups, then parameters,
    moments and step counts restored between the two runs).

    The 1x1-conv weight gradients are summed with fp32 atomics, so the two runs see gradients that differ in the last
    bits, and Adam's normalised update can turn such a difference into a full update of the other sign where a
    gradient component is noise (near-cancelling sums).  So the test checks two things that hold for certain:
    * every real: each run moves it by at most lr (R + wd |p|) per step, R = the Cauchy-Schwarz bound of
      |m^| / sqrt(v^) (``_adam_ratio_bound``), so the runs differ by at most 2 * 3 lr (R + wd |p|);
    * the signal: where, in every eager step, the gradient's RMS sqrt(v) is at least 1e-3 of its tensor's RMS and the
      moment |m| at least 1e-3 sqrt(v), a relative gradient difference of the atomics' order (< 1e-4 there) moves the
      update by far less than 1e-3 lr; those reals -- most of the net -- must agree to 5e-2 lr."""
    from makani_amd.optim import FusedAdamW
    from makani_amd.sfnonet import SphericalFourierNeuralOperatorNet
    torch.manual_seed(7)
    kw = dict(inp_shape=(32, 64), out_shape=(32, 64), scale_factor=2, inp_chans=4, out_chans=3, embed_dim=8, num_layers=2)
    lr, wd, betas, eps = 1e-3, 0.01, (0.9, 0.999), 1e-8
    x, tar = torch.randn(2, 4, 32, 64, device=dev), torch.randn(2, 3, 32, 64, device=dev)
    net = SphericalFourierNeuralOperatorNet(**kw).to(dev)
    params = [p for p in net.parameters()]
    opt = FusedAdamW(params, lr=lr, betas=betas, eps=eps, weight_decay=wd, max_grad_norm=1.0, capturable=True)
    static_inp, static_tar = x.clone(), tar.clone()

    def body():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = ((net(static_inp).float() - static_tar) ** 2).mean()
        loss.backward()
        opt.step()

    def real(t):
        return torch.view_as_real(t) if t.is_complex() else t

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                                    # shared warm-ups
            net.zero_grad(set_to_none=True)
            body()
        s.synchronize()
        snap = [(p.detach().clone(), opt.state[p]["m"].clone(), opt.state[p]["v"].clone(),
                 opt.state[p]["step"].clone()) for p in params]

        def restore():
            with torch.no_grad():
                for p, (p0, m0, v0, s0) in zip(params, snap):
                    p.copy_(p0)
                    opt.state[p]["m"].copy_(m0)
                    opt.state[p]["v"].copy_(v0)
                    opt.state[p]["step"].copy_(s0)

        signal = [torch.ones_like(real(p0), dtype=torch.bool) for p0, _, _, _ in snap]
        for _ in range(3):                                    # run A: eager
            net.zero_grad(set_to_none=True)
            body()
            for i, p in enumerate(params):
                m, v = real(opt.state[p]["m"]), real(opt.state[p]["v"])
                rms = v.sqrt()
                signal[i] &= (rms >= 1e-3 * rms.pow(2).mean().sqrt()) & (m.abs() >= 1e-3 * rms)
        s.synchronize()
        out_a = [real(p.detach()).clone() for p in params]
        restore()
        gc.collect()
        torch.cuda.empty_cache()
        graph = torch.cuda.CUDAGraph()                        # run B: one graph, replayed
        net.zero_grad(set_to_none=True)
        graph.capture_begin()
        body()
        graph.capture_end()
        for _ in range(3):
            graph.replay()
        s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    out_b = [real(p.detach()).clone() for p in params]
    R = max(_adam_ratio_bound(*betas, t) for t in (3, 4, 5))
    n_sig = n_all = 0
    moved = 0.0
    for (p0, _, _, _), a, b, sig, (name, _) in zip(snap, out_a, out_b, signal, net.named_parameters()):
        d = (a - b).abs()
        bound = 2 * 3 * lr * (R + wd * (real(p0).abs() + 0.01)) + 1e-7
        assert bool((d <= bound).all()), name
        assert bool((d[sig] <= 5e-2 * lr).all()), (name, d[sig].max().item() / lr)
        moved += (a - real(p0)).abs().sum().item()
        n_sig += int(sig.sum())
        n_all += sig.numel()
    assert moved > 0                                                          # the steps did move the net
    assert n_sig >= 0.25 * n_all, n_sig / n_all


def test_eager_step_invalidates_saved_parameters(dev):
    from makani_amd.optim import FusedAdamW
    p = torch.nn.Parameter(torch.randn(4096, device=dev))
    opt = FusedAdamW([p], lr=0.1)
    y = (p * p).sum()
    p.grad = torch.ones_like(p)
    opt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward()


def _offset_copy(src, off):
    """A copy of ``src`` (fp32, contiguous) that starts ``off`` floats into a fresh buffer."""
    buf = torch.zeros(src.numel() + 8, device=src.device)
    v = buf[off:off + src.numel()].view(src.shape)
    v.copy_(src)
    return v


@pytest.mark.parametrize("off", [1, 2])
@pytest.mark.parametrize("cls", ["FusedAdamW", "FusedLAMB"])
def test_streams_at_the_same_unaligned_offset(dev, cls, off):
    """p, g, m and v all 4 * off bytes past a 16-byte boundary: the kernels take the scalar head, float4 body and
    scalar tail of every chunk (4 chunks of 16 K reals and a tail here), and the result is the reference's."""
    from makani_amd import optim
    from test_optim_cpu import lamb_reference
    torch.manual_seed(3)
    shape = (257, 193)
    p0 = torch.randn(shape, device=dev)
    grads = [torch.randn(shape, device=dev) for _ in range(4)]
    p = torch.nn.Parameter(_offset_copy(p0, off))
    kw = dict(lr=1e-2, betas=(0.9, 0.95), weight_decay=0.1, max_grad_norm=50.0)
    opt = getattr(optim, cls)([p], **kw)
    opt.state[p] = {"m": _offset_copy(torch.zeros(shape, device=dev), off),
                    "v": _offset_copy(torch.zeros(shape, device=dev), off), "step": torch.tensor(0.0)}
    for g in grads:
        p.grad = _offset_copy(g, off)
        opt.step()
    for t in (p, p.grad, opt.state[p]["m"], opt.state[p]["v"]):
        assert t.data_ptr() % 16 == 4 * off
    if cls == "FusedAdamW":
        q = torch.nn.Parameter(p0.clone())
        topt = torch.optim.AdamW([q], lr=1e-2, betas=(0.9, 0.95), weight_decay=0.1)
        for g in grads:
            q.grad = g.clone()
            torch.nn.utils.clip_grad_norm_([q], 50.0)
            topt.step()
        want, want_m = q, topt.state[q]["exp_avg"]
    else:
        ref = [torch.nn.Parameter(p0.clone())]
        P, M, _ = lamb_reference(ref, [[g] for g in grads], 1e-2, (0.9, 0.95), 1e-6, 0.1, max_grad_norm=50.0)
        want, want_m = P[0], M[0]
    assert rel(p, want) <= TOL
    assert rel(opt.state[p]["m"], want_m) <= TOL


@pytest.mark.parametrize("cls", ["FusedAdamW", "FusedLAMB"])
def test_model_parallel_norm_path_captures_without_uploads(dev, cls, monkeypatch):
    """The norm path of sharded parameters (index vectors, per-group select / all-reduce / scatter) rebuilt INSIDE a
    captured region: a host-to-device copy there would fail the capture.  One rank stands in for the group (the
    all-reduce of one rank is the identity), so the replays must equal eager steps bit for bit."""
    import torch.distributed as dist
    from makani_amd import optim
    monkeypatch.setattr(optim, "_dist_ready", lambda: True)
    monkeypatch.setattr(optim, "_mp_names", lambda p: ["h"] if p.dim() >= 2 else [])
    monkeypatch.setattr(dist, "all_reduce", lambda t, op=None, group=None, async_op=False: None)
    x = torch.randn(32, 1001, device=dev)
    z = torch.randn(96, 96, 120, dtype=torch.complex64, device=dev)
    results = []
    for graphed in (False, True):
        ps = _synthetic(dev)
        opt = getattr(optim, cls)(ps, lr=1e-2, weight_decay=0.05, max_grad_norm=1.0, capturable=True)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(1 if graphed else 4):
                opt.zero_grad(set_to_none=True)
                _loss(ps, x, z).backward()
                optim.clip_grad_norm_(ps, 2.0)
                opt.step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        assert opt._plan["red"]                            # the model-parallel path is taken
        if graphed:
            opt._reducers.clear()                          # rebuilt during capture
            optim._REDUCERS.clear()
            g = torch.cuda.CUDAGraph()
            opt.zero_grad(set_to_none=True)
            with torch.cuda.graph(g):
                _loss(ps, x, z).backward()
                optim.clip_grad_norm_(ps, 2.0)
                opt.step()
            assert opt._plan["red"]
            for _ in range(3):
                g.replay()
        torch.cuda.synchronize()
        results.append([p.detach().clone() for p in ps])
    for a, b in zip(*results):
        assert torch.equal(a, b)
