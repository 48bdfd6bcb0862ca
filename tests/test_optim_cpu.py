"""CPU tests of the multi-tensor optimizers (makani_amd.optim: FusedAdamW, FusedLAMB, clip_grad_norm_): the torch
implementation of their arithmetic against torch's optimizers and a float64 restatement of apex FusedLAMB, the
torch.optim.Optimizer integration (schedulers, state_dict, GradScaler) and the model-parallel norms over gloo.
The kernels themselves are tested in test_optim_gpu.py with the same cases (the helpers below are shared)."""
import io
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import capi_checks as capi

TOL = 1e-6


def rel(a, b):
    a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    nb = torch.linalg.norm(b)
    return (torch.linalg.norm(a - b) / (nb if nb > 0 else 1.0)).item()


def make_params(device="cpu", big=False, seed=0):
    """A real matrix, a complex tensor, a permuted-contiguous complex [L][I][O] weight (public [I, O, L]), a small
    odd-length vector; with ``big`` also a production-size dhconv weight and a view at a 4-byte offset."""
    g = torch.Generator().manual_seed(seed)
    L, I, O = (240, 384, 384) if big else (7, 5, 6)
    ts = [torch.randn(33, 17, generator=g),
          torch.randn(9, 11, dtype=torch.complex64, generator=g),
          torch.randn(L, I, O, dtype=torch.complex64, generator=g).permute(1, 2, 0),
          torch.randn(13, generator=g)]
    if big:
        ts.append(torch.randn(1 << 20, generator=g) * 0.1)
        ts.append(torch.randn(5, 3, generator=g))
    ps = [torch.nn.Parameter(t.to(device)) for t in ts]
    if big:      # parameter that starts 4 bytes into its storage
        buf = torch.randn(4097 * 3 + 1, generator=g).to(device)
        ps.append(torch.nn.Parameter(buf[1:].view(4097, 3)))
    return ps


def make_grads(ps, steps, skip=(1, 1), seed=1, scale=1.0):
    """Per step a list of gradients (None where the parameter gets none: parameter skip[1] at step skip[0])."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in range(steps):
        gs = []
        for i, p in enumerate(ps):
            if skip is not None and (s, i) == tuple(skip):
                gs.append(None)
                continue
            t = torch.randn(p.shape, dtype=p.dtype, generator=g) * scale
            gs.append(t.to(p.device))
        out.append(gs)
    return out


def set_grads(ps, gs):
    for p, g in zip(ps, gs):
        if g is None:
            p.grad = None
        else:
            p.grad = torch.empty_like(p.data)        # the parameter's layout (as autograd produces it)
            p.grad.copy_(g)


def clone_params(ps):
    out = []
    for p in ps:
        q = torch.empty_like(p.data)
        q.copy_(p.data)
        out.append(torch.nn.Parameter(q))
    return out


def run(opt_fn, ps, grads):
    opt = opt_fn(ps)
    for gs in grads:
        set_grads(ps, gs)
        opt.step()
    return opt


def lamb_reference(ps, grads, lr, betas, eps, wd, adam_w_mode=True, grad_averaging=True, max_grad_norm=1.0,
                   use_nvlamb=False, bias_correction=True):
    """float64 restatement of apex FusedLAMB (fused_lamb.py + multi_tensor_lamb.cu), per-parameter step counts."""
    b1, b2 = betas
    b3 = 1.0 - b1 if grad_averaging else 1.0
    P = [(torch.view_as_real(p.data) if p.is_complex() else p.data).double().clone() for p in ps]
    M = [torch.zeros_like(x) for x in P]
    V = [torch.zeros_like(x) for x in P]
    steps = [0] * len(P)
    for gs in grads:
        G64 = [(torch.view_as_real(g) if g.is_complex() else g).double() if g is not None else None for g in gs]
        G = math.sqrt(sum((g ** 2).sum().item() for g in G64 if g is not None))
        c = G / max_grad_norm if (max_grad_norm and G > max_grad_norm) else 1.0
        us = []
        for i, g in enumerate(G64):
            if g is None:
                us.append(None)
                continue
            steps[i] += 1
            gh = g / c
            if not adam_w_mode:
                gh = gh + wd * P[i]
            M[i] = b1 * M[i] + b3 * gh
            V[i] = b2 * V[i] + (1 - b2) * gh * gh
            bc1, bc2 = (1 - b1 ** steps[i], 1 - b2 ** steps[i]) if bias_correction else (1.0, 1.0)
            u = (M[i] / bc1) / ((V[i] / bc2).sqrt() + eps)
            if adam_w_mode:
                u = u + wd * P[i]
            us.append(u)
        for i, u in enumerate(us):
            if u is None:
                continue
            pn, un = P[i].norm().item(), u.norm().item()
            r = lr * pn / un if (use_nvlamb or wd != 0) and pn != 0 and un != 0 else lr
            P[i] = P[i] - r * u
    return P, M, V


LAMB_CASES = [dict(wd=0.0, use_nvlamb=False, max_grad_norm=1.0),
              dict(wd=0.1, use_nvlamb=False, max_grad_norm=1.0),
              dict(wd=0.0, use_nvlamb=True, max_grad_norm=1.0),
              dict(wd=0.1, use_nvlamb=False, max_grad_norm=1e6),           # clip inactive
              dict(wd=0.1, use_nvlamb=True, max_grad_norm=2.0, grad_averaging=False),
              dict(wd=0.05, use_nvlamb=False, max_grad_norm=2.0, adam_w_mode=False)]


def check_adamw(device, adam_w_mode, big=False, max_grad_norm=None, capturable=False):
    from makani_amd.optim import FusedAdamW
    ps = make_params(device, big)
    ref = clone_params(ps)
    grads = make_grads(ps, 5)
    kw = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
    opt = run(lambda q: FusedAdamW(q, adam_w_mode=adam_w_mode, max_grad_norm=max_grad_norm, capturable=capturable, **kw),
              ps, grads)
    tcls = torch.optim.AdamW if adam_w_mode else torch.optim.Adam
    topt = tcls(ref, **kw)
    for gs in grads:
        set_grads(ref, gs)
        if max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_([p for p in ref if p.grad is not None], max_grad_norm)
        topt.step()
    for p, q in zip(ps, ref):
        assert rel(p, q) <= TOL
        assert rel(opt.state[p]["m"], topt.state[q]["exp_avg"]) <= TOL
        assert rel(opt.state[p]["v"], topt.state[q]["exp_avg_sq"]) <= TOL
        assert float(opt.state[p]["step"]) == float(topt.state[q]["step"])
    return opt, ps


def check_lamb(device, case, big=False, capturable=False):
    from makani_amd.optim import FusedLAMB
    case = dict(case)
    wd = case.pop("wd")
    ps = make_params(device, big)
    grads = make_grads(ps, 5, skip=None, scale=0.5)
    kw = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-6, weight_decay=wd, **case)
    P, M, V = lamb_reference(ps, grads, kw["lr"], kw["betas"], kw["eps"], wd,
                             **{k: case[k] for k in case})
    opt = run(lambda q: FusedLAMB(q, capturable=capturable, **kw), ps, grads)
    for p, pr, mr, vr in zip(ps, P, M, V):
        assert rel(p, pr) <= TOL
        assert rel(opt.state[p]["m"], mr) <= TOL
        assert rel(opt.state[p]["v"], vr) <= TOL
    return opt, ps


@pytest.mark.parametrize("adam_w_mode", [True, False])
def test_fused_adamw_matches_torch(adam_w_mode):
    check_adamw("cpu", adam_w_mode)


def test_fused_adamw_max_grad_norm_matches_torch_clip():
    check_adamw("cpu", True, max_grad_norm=5.0)


@pytest.mark.parametrize("case", LAMB_CASES)
def test_fused_lamb_matches_apex_arithmetic(case):
    check_lamb("cpu", case)


def test_lamb_rejects_amsgrad():
    from makani_amd.optim import FusedLAMB
    with pytest.raises(RuntimeError):
        FusedLAMB([torch.nn.Parameter(torch.zeros(3))], amsgrad=True)


def test_clip_grad_norm_matches_torch():
    from makani_amd.optim import clip_grad_norm_
    for max_norm in (1.0, 1e6):
        ps = make_params()
        ref = clone_params(ps)
        gs = make_grads(ps, 1, skip=None)[0]
        set_grads(ps, gs)
        set_grads(ref, gs)
        n = clip_grad_norm_(ps, max_norm)
        nr = torch.nn.utils.clip_grad_norm_(ref, max_norm)
        assert isinstance(n, torch.Tensor) and n.dim() == 0
        assert abs(n.item() - nr.item()) <= TOL * nr.item()
        for p, q in zip(ps, ref):
            assert rel(p.grad, q.grad) <= TOL


@pytest.mark.parametrize("cls", ["FusedAdamW", "FusedLAMB"])
def test_schedulers_and_grad_scaler(cls):
    from makani_amd import optim
    ps = make_params()
    opt = getattr(optim, cls)(ps, lr=0.1)
    assert isinstance(opt, torch.optim.Optimizer)
    for sched in (torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5),
                  torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=4)):
        for gs in make_grads(ps, 3, skip=None):
            set_grads(ps, gs)
            torch.amp.GradScaler("cpu", enabled=False).step(opt)
            sched.step()
    assert opt.param_groups[0]["lr"] != 0.1


@pytest.mark.parametrize("cls", ["FusedAdamW", "FusedLAMB"])
def test_state_dict_round_trip(cls):
    from makani_amd import optim
    kw = dict(lr=1e-2, weight_decay=0.1)
    ps = make_params()
    grads = make_grads(ps, 6, skip=None)
    opt = getattr(optim, cls)(ps, **kw)
    for gs in grads[:3]:
        set_grads(ps, gs)
        opt.step()
    buf = io.BytesIO()                 # through a checkpoint file, as the trainer does
    torch.save(opt.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=False)
    ps2 = clone_params(ps)
    opt2 = getattr(optim, cls)(ps2, **kw)
    opt2.load_state_dict(sd)
    for gs in grads[3:]:
        for q, o in ((ps, opt), (ps2, opt2)):
            set_grads(q, gs)
            o.step()
    for p, q in zip(ps, ps2):
        assert torch.equal(p, q)
        assert torch.equal(opt.state[p]["m"], opt2.state[q]["m"])


def test_step_bumps_the_parameter_version():
    from makani_amd.optim import FusedAdamW
    p = torch.nn.Parameter(torch.randn(8))
    opt = FusedAdamW([p], lr=0.1)
    y = (p * p).sum()              # saves p
    p.grad = torch.ones(8)
    opt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward()


# ------------------------------------------------------------------ world 2 over gloo, h = 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _mp_model(seed=3):
    """[sharded over h along dim 0, shared (is_shared_mp)], full (logical) tensors."""
    g = torch.Generator().manual_seed(seed)
    full = [torch.randn(10, 6, generator=g), torch.randn(7, generator=g)]
    grads = [[torch.randn(10, 6, generator=g) * 2, torch.randn(7, generator=g) * 2] for _ in range(4)]
    return full, grads


def _opt_for(name, ps):
    from makani_amd.optim import FusedAdamW, FusedLAMB
    if name == "lamb":
        return FusedLAMB(ps, lr=1e-2, weight_decay=0.1, max_grad_norm=1.0)      # the clip is active (|g| ~ 20)
    return FusedAdamW(ps, lr=1e-2, weight_decay=0.1, max_grad_norm=1.0)


def _mp_worker(rank, world, port, name, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        torch.set_num_threads(1)
        from makani_amd import comm
        comm.init(model_parallel_sizes=[world, 1, 1, 1], backend="gloo")
        full, grads = _mp_model()
        h, r = comm.get_size("h"), comm.get_rank("h")
        rows = 10 // h
        sh = torch.nn.Parameter(full[0][r * rows:(r + 1) * rows].clone())
        sh.sharded_dims_mp = ["h", None]
        sh.is_shared_mp = []
        shared = torch.nn.Parameter(full[1].clone())
        shared.is_shared_mp = ["h"]
        opt = _opt_for(name, [sh, shared])
        for gs in grads:
            sh.grad = gs[0][r * rows:(r + 1) * rows].clone()
            shared.grad = gs[1].clone()
            opt.step()
        outs = [torch.empty_like(sh.data) for _ in range(h)]
        dist.all_gather(outs, sh.data.contiguous(), group=comm.get_group("h"))
        sh_full = torch.cat(outs, 0)
        others = [torch.empty_like(shared.data) for _ in range(h)]
        dist.all_gather(others, shared.data, group=comm.get_group("h"))
        # single process
        ps = [torch.nn.Parameter(t.clone()) for t in full]
        o1 = _opt_for(name, ps)
        for gs in grads:
            for p, g in zip(ps, gs):
                p.grad = g.clone()
            o1.step()
        assert rel(sh_full, ps[0]) <= TOL, rel(sh_full, ps[0])
        assert rel(shared, ps[1]) <= TOL, rel(shared, ps[1])
        assert all(torch.equal(o, others[0]) for o in others)
        dist.barrier()
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("name", ["lamb", "adamw"])
def test_model_parallel_norms_h2(name):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mp_worker, args=(r, 2, port, name, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    bad = [r for r in results if r[1] != "ok"]
    assert not bad, "\n".join(f"rank {r}: {m}" for r, m in bad)


def test_reducer_index_runs(monkeypatch):
    """The per-group index vector of the model-parallel norm reduction, built from arange runs (no host copy)."""
    from makani_amd import optim
    monkeypatch.setattr(optim, "_dist_ready", lambda: True)
    ps = [torch.zeros(2, 2), torch.zeros(3), torch.zeros(2, 2), torch.zeros(1, 1), torch.zeros(4), torch.zeros(5, 1)]
    monkeypatch.setattr(optim, "_mp_names", lambda p: ["h"] + (["w"] if p.numel() == 1 else []) if p.dim() == 2 else [])
    red = optim._Reducer(ps, torch.device("cpu"))
    plan = {n: idx.tolist() for n, idx, _ in red.plan}
    assert plan == {"h": [0, 2, 3, 5], "w": [3]}
    cache = {}
    assert optim._reducer_for(ps, torch.device("cpu"), cache) is optim._reducer_for(ps, torch.device("cpu"), cache)


# ---------------------------------------------------------------------------------------------------------------------
# misaligned pointers: refused by the host checks, with the message of the check (tests/capi_checks.py)
# ---------------------------------------------------------------------------------------------------------------------
_A = capi.A
MISALIGNED = [      # entry point, its arguments in front of the stream with one pointer moved off its alignment, the refusal
    ("mk_adam_step", (_A, _A, _A, _A + 4, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1), "buffers must be 16-byte aligned"),
    ("mk_adam_step", (_A, _A + 8, _A, _A, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1), "buffers must be 16-byte aligned"),
]


@pytest.mark.parametrize("case", MISALIGNED, ids=capi.case_ids(MISALIGNED))
def test_misaligned_pointer_is_refused_before_any_launch(case):
    capi.assert_refused(*case)
