"""Single-pass Adam over the model's parameters, complex ones included.

The reference patches torch's Adam for complex parameters (``makani/third_party/torch``) and
steps outside the captured graph (``makani/utils/trainer.py:762-763``).  Adam treats a complex
number as two reals, so every parameter is stepped through a real view of its storage
(complex64 -> ``view_as_real``):

* large dense tensors (the spectral weights: 283 M of the net's 289 M parameters) by
  ``mk_adam_step`` -- one HIP streaming pass per tensor over its storage in memory order;
* the many small ones by ``torch.optim.Adam(fused=True)`` in one multi-tensor launch.

``overlap_backward=k`` (opt-in, 0 = off): the update of a large tensor is launched on a side stream as soon as its gradient
has been accumulated ``k`` times in this step (``k`` = backward passes per step: 1, or the number of micro-batches), so the
HBM-bound streaming pass runs under the remaining backward kernels (which leave most of the HBM bandwidth idle) instead
of after them; ``step()`` launches whatever is left and joins the side stream.  The arithmetic and the result are the same
as without it.  (On one MI355X the step time does not change: the backward kernels that run beside an Adam pass slow
down by what the pass would have cost alone -- ``bench.py`` leaves it off.)  Only valid when nothing is done to these gradients between backward and ``step()``: no gradient clipping
or scaling, no data-parallel averaging (the spectral weights are sharded, not shared, over the model-parallel groups, so
``reduce_shared_gradients`` does not touch them).  Under stream capture the hook does nothing (the captured graph ends with
backward; the optimizer steps outside it, ``trainer.py:762-763``).
"""
import math

import torch

from . import _lib

_BIG = 1 << 20      # elements: below this the per-tensor launch is not worth it


def _flat_storage_view(t):
    """1-D view over a dense tensor's elements in memory order (works for permuted-contiguous layouts), or None."""
    if t.is_contiguous():
        return t.view(-1)
    order = sorted(range(t.dim()), key=lambda d: -t.stride(d))
    tp = t.permute(order)
    return tp.reshape(-1) if tp.is_contiguous() else None


class FusedAdam:
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, overlap_backward=0):
        self.params = [p for p in params if p.requires_grad]
        self.defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.views, self._small, self._big = [], [], []
        self.overlap_backward = int(overlap_backward)
        self._side = None           # side stream of the overlapped updates
        self._hooks = []
        for p in self.params:
            v = (torch.view_as_real(p.data) if p.is_complex() else p.data).detach()
            self.views.append(v)
            flat = _flat_storage_view(v) if (v.is_cuda and v.dtype == torch.float32 and v.numel() >= _BIG) else None
            if flat is not None and flat.data_ptr() % 16 == 0:
                st = {"p": p, "flat": flat, "m": torch.zeros_like(flat), "v": torch.zeros_like(flat), "step": 0,
                      "acc": 0, "done": False}
                self._big.append(st)
                if self.overlap_backward > 0:
                    self._hooks.append(p.register_post_accumulate_grad_hook(lambda _p, st=st: self._grad_ready(st)))
            else:
                self._small.append((p, v))
        self.opt = None
        self._own_groups = [dict(self.defaults, params=[])]
        if self._small:
            self.opt = torch.optim.Adam([v for _, v in self._small], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                        fused=all(v.is_cuda for _, v in self._small))

    @property
    def param_groups(self):
        """ONE persistent list (torch's for the small tensors, else the optimizer's own): a scheduler that writes
        ``group["lr"]`` reaches both the torch optimizer and the streaming passes, which read group 0."""
        return self.opt.param_groups if self.opt is not None else self._own_groups

    def zero_grad(self, set_to_none=True):
        for st in self._big:
            st["acc"] = 0
        for p, v in zip(self.params, self.views):
            v.grad = None
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    @staticmethod
    def _grad_like_param(p):
        g = p.grad
        if g is not None and g.stride() != p.stride():      # the kernels walk storage linearly: layouts must agree
            g2 = torch.empty_like(p.data)                    # preserve_format -> the parameter's strides
            g2.copy_(g)
            g = g2
        return g

    def _step_big(self, st, stream):
        """One streaming pass over a large tensor on ``stream`` (a raw HIP stream handle)."""
        g = self._grad_like_param(st["p"])
        if g is None:
            return
        hp = self.param_groups[0]
        lr, (b1, b2), eps, wd = hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"]
        gf = _flat_storage_view(torch.view_as_real(g) if g.is_complex() else g)
        assert gf is not None and gf.dtype == torch.float32 and gf.numel() == st["flat"].numel()
        st["step"] += 1
        _lib.check(_lib.load().mk_adam_step(st["flat"].data_ptr(), gf.data_ptr(), st["m"].data_ptr(), st["v"].data_ptr(),
                                            gf.numel(), float(lr), float(b1), float(b2), float(eps), float(wd), st["step"],
                                            stream), "mk_adam_step")

    def _grad_ready(self, st):
        """Post-accumulate hook of a large tensor (``overlap_backward``): after the last accumulation of the step its update
        goes to the side stream, ordered behind everything the accumulating stream has queued so far (the kernels that read
        the old weights and wrote the gradient)."""
        st["acc"] += 1
        if st["acc"] != self.overlap_backward or st["done"] or not st["p"].is_cuda:
            return
        if torch.cuda.is_current_stream_capturing():
            return
        if self._side is None:
            self._side = torch.cuda.Stream(device=st["p"].device)    # gfx950 offers priorities (0, -1): 0 is the lowest
        self._side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._side):
            self._step_big(st, self._side.cuda_stream)
        st["done"] = True

    def step(self):
        for p, v in self._small:
            g = self._grad_like_param(p)
            v.grad = None if g is None else (torch.view_as_real(g) if g.is_complex() else g)
        if self.opt is not None:
            self.opt.step()
        if not self._big:
            return
        stream = torch.cuda.current_stream().cuda_stream
        joined = False
        for st in self._big:
            if st["done"]:              # already under way on the side stream: the gradient stays alive until the join below
                st["done"] = False
                joined = True
            else:
                self._step_big(st, stream)
            st["acc"] = 0
        if joined:
            torch.cuda.current_stream().wait_stream(self._side)

    def state_dict(self):
        return {"small": None if self.opt is None else self.opt.state_dict(),
                "big": [{"m": st["m"], "v": st["v"], "step": st["step"]} for st in self._big]}

    def load_state_dict(self, sd):
        if not isinstance(sd, dict) or set(sd) != {"small", "big"}:
            raise ValueError("FusedAdam.load_state_dict: unrecognised layout (expected keys {'small', 'big'}; a plain "
                             "torch.optim.Adam state dict cannot be mapped onto the split small / large tensor state)")
        if len(sd["big"]) != len(self._big):
            raise ValueError(f"FusedAdam.load_state_dict: {len(sd['big'])} large-tensor states for {len(self._big)} tensors")
        if self.opt is not None and sd.get("small") is not None:
            self.opt.load_state_dict(sd["small"])
        for st, src in zip(self._big, sd.get("big", [])):
            st["m"].copy_(src["m"])
            st["v"].copy_(src["v"])
            st["step"] = int(src["step"])


# ====================================================================== multi-tensor optimizers (optim.hip)
# FusedAdamW / FusedLAMB / clip_grad_norm_: the optimizers of the reference trainer's ``optimizer_type`` switch
# (makani/utils/trainer.py:448-478: torch AdamW / Adam, apex FusedLAMB) and its ``max_grad_norm`` clipping, as
# torch.optim.Optimizer subclasses (LR schedulers, GradScaler and state_dict work as with torch's optimizers).
#
# One launch sequence per step covers every tensor: the tensor list goes to the kernels by value, so the step can be
# captured into a graph.  With ``capturable=True`` the learning rate (group["lr"], a 0-dim fp32 device tensor that
# torch's schedulers update with fill_) and the step counts (a float32 device table; state["step"] is a 0-dim view
# of it) live on the device, and step() only launches.
#
# Norms are those of the logical (unsharded) model: the per-tensor sums of squares of parameters sharded over a
# model-parallel group (``sharded_dims_mp``) are summed over that group with one all-reduce per group, and shared
# parameters (``is_shared_mp``, made equal by the gradient reduction) count once.  This deviates from apex, whose
# LAMB would clip every shard with its own norm.  CPU tensors take a torch implementation of the same arithmetic.

def _real(t):
    return torch.view_as_real(t) if t.is_complex() else t


def _flat_real(t, what):
    f = _flat_storage_view(_real(t))
    if f is None or f.dtype != torch.float32:
        raise TypeError(f"makani_amd.optim: {what} must be a dense fp32 / complex64 tensor (got {t.dtype}, "
                        f"shape {tuple(t.shape)}, strides {t.stride()})")
    return f


def _grad_like(p, bufs=None):
    """The gradient in the parameter's layout (the kernels walk both linearly in memory order).  A gradient whose
    strides differ is copied into a buffer kept per parameter in ``bufs``, so its address stays the same."""
    g = p.grad
    if g.stride() != p.stride():
        g2 = None if bufs is None else bufs.get(p)
        if g2 is None:
            g2 = torch.empty_like(p.data)
            if bufs is not None:
                bufs[p] = g2
        g2.copy_(g)
        g = g2
    return g


def _mp_names(p):
    """Model-parallel groups (of size > 1) the parameter is sharded over."""
    from . import comm
    names = []
    for n in getattr(p, "sharded_dims_mp", None) or []:
        if n is not None and n not in names and comm.get_size(n) > 1:
            names.append(n)
    return names


def _u64(vals):
    import ctypes
    return (ctypes.c_uint64 * len(vals))(*vals)


def _i64(vals):
    import ctypes
    return (ctypes.c_longlong * len(vals))(*vals)


def _i32(vals):
    import ctypes
    return (ctypes.c_int * max(1, len(vals)))(*vals)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dist_ready():
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized()


class _Reducer:
    """Sums per-tensor norm vectors over the model-parallel groups the tensors are sharded over.

    The index vectors are built on the device from ``arange`` runs (no host-to-device copy), so a reducer may be built
    inside a captured region; the optimizers and ``clip_grad_norm_`` also cache it per parameter set."""

    def __init__(self, params, device):
        self.plan = []          # (group name, index tensor, buffer)
        if not _dist_ready():
            return
        by = {}
        for i, p in enumerate(params):
            for n in _mp_names(p):
                by.setdefault(n, []).append(i)
        for n, idx in by.items():
            runs, a = [], idx[0]
            for j in range(1, len(idx) + 1):
                if j == len(idx) or idx[j] != idx[j - 1] + 1:
                    runs.append(torch.arange(a, idx[j - 1] + 1, dtype=torch.long, device=device))
                    a = idx[j] if j < len(idx) else None
            self.plan.append((n, runs[0] if len(runs) == 1 else torch.cat(runs),
                              torch.empty(len(idx), dtype=torch.float64, device=device)))

    def __bool__(self):
        return bool(self.plan)

    def __call__(self, *vecs):
        import torch.distributed as dist
        from . import comm
        for n, idx, buf in self.plan:
            for v in vecs:
                torch.index_select(v, 0, idx, out=buf)
                dist.all_reduce(buf, group=comm.get_group(n))
                v.index_copy_(0, idx, buf)


_REDUCERS = {}      # clip_grad_norm_: parameter set -> reducer (a few recent sets)


def _reducer_for(params, device, cache):
    import weakref
    key = (device, tuple(id(p) for p in params))
    red = cache.get(key)
    if red is None or any(r() is not p for r, p in zip(red[1], params)):     # ids of freed tensors can be reused
        if len(cache) >= 8:
            cache.pop(next(iter(cache)))
        red = cache[key] = (_Reducer(params, device), [weakref.ref(p) for p in params])
    return red[0]


def _sumsq_cpu(ts):
    return torch.stack([(_real(t).double() ** 2).sum() for t in ts]) if ts else torch.zeros(0, dtype=torch.float64)


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False):
    """``torch.nn.utils.clip_grad_norm_`` on the multi-tensor kernels: the gradients are rescaled in place by
    min(1, max_norm / (total + 1e-6)) and the total norm comes back as a 0-dim device tensor, never read on the host.
    The norm is that of the logical model under model parallelism (see above).  Other ``norm_type`` go to torch."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    if not params:
        return torch.tensor(0.0)
    if float(norm_type) != 2.0:
        return torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type, error_if_nonfinite)
    grads = [p.grad for p in params]
    dev = grads[0].device
    red = _reducer_for(params, dev, _REDUCERS)
    if dev.type != "cuda":
        tsum = _sumsq_cpu(grads)
        if red:
            red(tsum)
        total = tsum.sum().sqrt().float()
        coef = torch.clamp(float(max_norm) / (total + 1e-6), max=1.0)
        for g in grads:
            _real(g).mul_(coef)
    else:
        flats = [_flat_real(g, "a gradient") for g in grads]
        ptrs, ns = _u64([f.data_ptr() for f in flats]), _i64([f.numel() for f in flats])
        lib = _lib.load()
        nch = sum(lib.mk_mt_chunks(f.numel()) for f in flats)
        ws = torch.empty(nch + len(flats), dtype=torch.float64, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        partials, tsum = ws[:nch], ws[nch:]
        total, coef = out[0], out[1:]
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.mk_mt_sumsq(len(flats), ptrs, ns, partials.data_ptr(), tsum.data_ptr(), 0 if red else 1,
                                   float(max_norm), total.data_ptr(), coef.data_ptr(), None, None, 0, stream), "mk_mt_sumsq")
        if red:
            red(tsum)
            _lib.check(lib.mk_mt_norm_finish(len(flats), tsum.data_ptr(), 1, float(max_norm), total.data_ptr(),
                                             coef.data_ptr(), None, None, 0, stream), "mk_mt_norm_finish")
        _lib.check(lib.mk_mt_scale(len(flats), ptrs, ns, coef.data_ptr(), stream), "mk_mt_scale")
    if error_if_nonfinite and not torch.isfinite(total):
        raise RuntimeError(f"The total norm of order {norm_type} for gradients is non-finite")
    return total


class _MultiTensorOptimizer(torch.optim.Optimizer):
    """Shared plumbing of FusedAdamW / FusedLAMB: state, device step table, workspaces, model-parallel norms."""

    def __init__(self, params, defaults, capturable):
        super().__init__(params, dict(defaults, capturable=bool(capturable)))
        self.capturable = bool(capturable)
        self._steps = None      # capturable: float32 device table, one slot per parameter
        self._plan = None       # cached launch arguments (keyed by the pointers)
        self._reducers = {}     # parameter set -> model-parallel reducer
        self._grad_bufs = {}    # parameter -> gradient copy in the parameter's layout (when autograd's differs)
        if self.capturable:
            dev = self._device()
            if dev.type != "cuda":
                raise ValueError(f"{type(self).__name__}(capturable=True) needs parameters on the GPU")
            for g in self.param_groups:
                g["lr"] = torch.tensor(float(g["lr"]), dtype=torch.float32, device=dev)
            self._steps = torch.zeros(len(self._all_params()), dtype=torch.float32, device=dev)

    def _all_params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _device(self):
        return self._all_params()[0].device

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if getattr(self, "capturable", False):
            g = self.param_groups[-1]
            if not isinstance(g["lr"], torch.Tensor):
                g["lr"] = torch.tensor(float(g["lr"]), dtype=torch.float32, device=self._device())
            old = self._steps
            self._steps = torch.zeros(len(self._all_params()), dtype=torch.float32, device=self._device())
            self._steps[:old.numel()].copy_(old)
            self._rebind_steps()

    def _rebind_steps(self):
        if self._steps is None:
            return
        for i, p in enumerate(self._all_params()):
            st = self.state.get(p)
            if st and "step" in st:
                if st["step"].data_ptr() != self._steps[i].data_ptr():
                    self._steps[i].copy_(st["step"])
                st["step"] = self._steps[i]

    def load_state_dict(self, state_dict):
        old_lr = [g["lr"] for g in self.param_groups]
        old_state = {p: dict(s) for p, s in self.state.items()}
        super().load_state_dict(state_dict)
        for g, lr in zip(self.param_groups, old_lr):
            if isinstance(lr, torch.Tensor):          # keep the tensor a captured graph reads
                lr.fill_(float(g["lr"]))
                g["lr"] = lr
        for p, st in self.state.items():              # and the moments it writes, when their layout agrees
            old = old_state.get(p, {})
            for k in ("m", "v"):
                if k in old and k in st and old[k].shape == st[k].shape and old[k].stride() == st[k].stride():
                    old[k].copy_(st[k])
                    st[k] = old[k]
        self._rebind_steps()
        self._plan = None

    def _init_state(self, p, slot):
        st = self.state[p]
        if "step" not in st:
            st["m"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["v"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if self._steps is not None:
                self._steps[slot].zero_()
                st["step"] = self._steps[slot]
            else:
                st["step"] = torch.tensor(0.0)
        return st

    def _collect(self):
        """[(group, [(slot, p, g)])] of the parameters that have a gradient, in group order."""
        out, slot = [], 0
        for g in self.param_groups:
            items = []
            for p in g["params"]:
                if p.grad is not None:
                    if p.grad.is_sparse:
                        raise RuntimeError(f"{type(self).__name__} does not support sparse gradients")
                    items.append((slot, p, _grad_like(p, self._grad_bufs)))
                slot += 1
            out.append((g, items))
        return out

    def _gpu_plan(self, groups, lamb):
        """Launch arguments and workspaces, cached while the pointers stay the same (no allocation after the first
        step of a stable parameter / gradient set)."""
        key = tuple((slot, p.data_ptr(), gr.data_ptr()) for _, items in groups for slot, p, gr in items)
        if self._plan is not None and self._plan["key"] == key:
            return self._plan
        lib = _lib.load()
        dev = self._device()
        plan = {"key": key, "groups": []}
        all_g, all_n, all_p, slots = [], [], [], []
        for g, items in groups:
            if not items:
                continue
            pgmv, ns, aux, ps = [], [], [], []
            for slot, p, gr in items:
                st = self.state[p]
                fl = [_flat_real(t, w) for t, w in ((p.data, "a parameter"), (gr, "a gradient"), (st["m"], "state"),
                                                    (st["v"], "state"))]
                if len({f.numel() for f in fl}) != 1:
                    raise RuntimeError("makani_amd.optim: parameter, gradient and state sizes differ")
                pgmv += [f.data_ptr() for f in fl]
                ns.append(fl[0].numel())
                aux.append(slot)
                ps.append(p)
                all_g.append(fl[1].data_ptr())
            all_n += ns
            all_p += ps
            slots += aux
            plan["groups"].append({"group": g, "params": ps, "T": len(ns), "pgmv": _u64(pgmv), "n": _i64(ns),
                                   "slots": _i32(aux), "off": len(all_n) - len(ns)})
        T = len(all_n)
        nch = sum(lib.mk_mt_chunks(n) for n in all_n)
        plan.update(T=T, g=_u64(all_g), n=_i64(all_n), slots=_i32(slots), nslots=len(slots), params=all_p)
        plan["partials"] = torch.empty((2 if lamb else 1) * max(nch, 1), dtype=torch.float64, device=dev)
        plan["tsum"] = torch.zeros(3 * T, dtype=torch.float64, device=dev)      # grads | LAMB |p|^2 | LAMB |u|^2
        plan["scal"] = torch.zeros(2, dtype=torch.float32, device=dev)          # total norm | clip coefficient
        plan["nch"] = nch
        plan["red"] = _reducer_for(all_p, dev, self._reducers)
        self._plan = plan
        return plan

    def _host_steps(self, items):
        aux = []
        for _, p, _g in items:
            st = self.state[p]
            st["step"] += 1
            aux.append(int(st["step"].item()))
        return _i32(aux)

    def _grad_norm(self, plan, clip_mode, max_norm, stream):
        """Gradient norm and clip coefficient into plan["scal"]; increments the device step table on the way."""
        lib = _lib.load()
        T, tsum = plan["T"], plan["tsum"]
        scal = plan["scal"]
        steps = _ptr(self._steps)
        ninc = plan["nslots"] if steps else 0
        red = plan["red"]
        _lib.check(lib.mk_mt_sumsq(T, plan["g"], plan["n"], plan["partials"].data_ptr(), tsum.data_ptr(),
                                   0 if red else clip_mode, float(max_norm), scal.data_ptr(), scal[1:].data_ptr(),
                                   None if red else steps, plan["slots"], 0 if red else ninc, stream), "mk_mt_sumsq")
        if red:
            red(tsum[:T])
            _lib.check(lib.mk_mt_norm_finish(T, tsum.data_ptr(), clip_mode, float(max_norm), scal.data_ptr(),
                                             scal[1:].data_ptr(), steps, plan["slots"], ninc, stream), "mk_mt_norm_finish")

    def _step_inc(self, plan, stream):
        if self._steps is not None:
            _lib.check(_lib.load().mk_mt_step_inc(self._steps.data_ptr(), plan["slots"], plan["nslots"], stream),
                       "mk_mt_step_inc")

    def _lr(self, g):
        lr = g["lr"]
        if self.capturable:
            return 0.0, lr.data_ptr()
        return float(lr), None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        if capturing and not self.capturable:
            raise RuntimeError(f"{type(self).__name__}: capturing a step needs capturable=True (the step count and lr "
                               "would be frozen into the graph)")
        groups = self._collect()
        params = [p for _, items in groups for _, p, _ in items]
        if not params:
            return loss
        for _, items in groups:
            for slot, p, _ in items:
                self._init_state(p, slot)
        if params[0].device.type == "cuda":
            self._step_gpu(groups)
        else:
            self._step_cpu(groups)
        if not capturing:
            torch.autograd.graph.increment_version(params)    # a tensor saved before the step now fails loudly
        return loss

    # CPU: the same arithmetic in torch (float64 norms), used where there is no GPU (and by the distributed tests)
    def _cpu_norm(self, groups):
        ps = [p for _, items in groups for _, p, _ in items]
        tsum = _sumsq_cpu([gr for _, items in groups for _, _, gr in items])
        red = _reducer_for(ps, torch.device("cpu"), self._reducers)
        if red:
            red(tsum)
        return float(tsum.sum().sqrt().float())

    def _cpu_steps(self, items):
        out = []
        for _, p, _ in items:
            self.state[p]["step"] += 1
            out.append(int(self.state[p]["step"].item()))
        return out


class FusedAdamW(_MultiTensorOptimizer):
    """torch.optim.AdamW (``adam_w_mode=True``: decoupled decay p *= 1 - lr wd) or torch.optim.Adam
    (``adam_w_mode=False``: L2 decay g += wd p) as one streaming pass over every tensor (``mk_mt_adam``).

    ``max_grad_norm`` folds torch's clip_grad_norm_ into the step: the gradients are multiplied by
    min(1, max_grad_norm / (|g| + 1e-6)) as they are read, and are left as they were."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, adam_w_mode=True,
                 max_grad_norm=None, capturable=False):
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        self.adam_w_mode = bool(adam_w_mode)
        self.max_grad_norm = max_grad_norm
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay), capturable)

    def _step_gpu(self, groups):
        lib = _lib.load()
        plan = self._gpu_plan(groups, lamb=False)
        stream = torch.cuda.current_stream(self._device()).cuda_stream
        clip = self.max_grad_norm is not None and self.max_grad_norm > 0
        if clip:
            self._grad_norm(plan, 1, self.max_grad_norm, stream)
        elif self.capturable:
            self._step_inc(plan, stream)
        coef = plan["scal"][1:].data_ptr() if clip else None
        for gp in plan["groups"]:
            g = gp["group"]
            aux = gp["slots"] if self.capturable else self._host_steps([(None, p, None) for p in gp["params"]])
            lr, lr_dev = self._lr(g)
            b1, b2 = g["betas"]
            _lib.check(lib.mk_mt_adam(gp["T"], gp["pgmv"], gp["n"], aux, _ptr(self._steps), lr, lr_dev, float(b1), float(b2),
                                      float(g["eps"]), float(g["weight_decay"]), int(self.adam_w_mode), coef, stream),
                       "mk_mt_adam")

    def _step_cpu(self, groups):
        coef = 1.0
        if self.max_grad_norm is not None and self.max_grad_norm > 0:
            total = torch.tensor(self._cpu_norm(groups), dtype=torch.float32)
            coef = float(torch.clamp(float(self.max_grad_norm) / (total + 1e-6), max=1.0))
        for g, items in groups:
            lr, (b1, b2), eps, wd = float(g["lr"]), g["betas"], g["eps"], g["weight_decay"]
            for (_, p, gr), step in zip(items, self._cpu_steps(items)):
                st = self.state[p]
                pr, m, v = _real(p.data), _real(st["m"]), _real(st["v"])
                gv = _real(gr) * coef
                if self.adam_w_mode:
                    pr.mul_(1.0 - lr * wd)
                else:
                    gv = gv + wd * pr
                m.mul_(b1).add_(gv, alpha=1.0 - b1)
                v.mul_(b2).addcmul_(gv, gv, value=1.0 - b2)
                bc1 = 1.0 - b1 ** step
                bc2s = math.sqrt(1.0 - b2 ** step)
                pr.addcdiv_(m, v.sqrt().div_(bc2s).add_(eps), value=-lr / bc1)


class FusedLAMB(_MultiTensorOptimizer):
    """apex ``FusedLAMB`` (apex/optimizers/fused_lamb.py, csrc/multi_tensor_lamb.cu) with apex's signature, so the
    reference's call (makani/utils/trainer.py:472) works unchanged.  Global gradient norm G, divisor
    c = G / max_grad_norm when G > max_grad_norm (``max_grad_norm`` None or 0: no clipping), moments of g / c,
    update u = m^ / (sqrt(v^) + eps) (+ wd p in adam_w_mode), trust ratio lr |p| / |u| when ``use_nvlamb`` or
    wd != 0.  Three documented deviations from apex: the gradient buffer is not overwritten with u; the norms are
    those of the logical model under model parallelism; and the step count behind the bias corrections is kept per
    parameter (``state[p]["step"]``, as torch's optimizers keep it), where apex keeps one per group and advances it
    even for a parameter without a gradient.  The two agree whenever every parameter of a group gets a gradient in
    every step, which is what the trainer does (``find_unused_parameters=False``)."""

    def __init__(self, params, lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01,
                 amsgrad=False, adam_w_mode=True, grad_averaging=True, set_grad_none=True, max_grad_norm=1.0,
                 use_nvlamb=False, capturable=False):
        if amsgrad:
            raise RuntimeError("FusedLAMB does not support the AMSGrad variant.")
        self.adam_w_mode = bool(adam_w_mode)
        self.set_grad_none = bool(set_grad_none)
        self.use_nvlamb = bool(use_nvlamb)
        super().__init__(params, dict(lr=lr, bias_correction=bias_correction, betas=tuple(betas), eps=eps,
                                      weight_decay=weight_decay, grad_averaging=grad_averaging,
                                      max_grad_norm=max_grad_norm), capturable)

    def zero_grad(self, set_to_none=None):
        super().zero_grad(set_to_none=self.set_grad_none if set_to_none is None else set_to_none)

    def _clip(self):
        mg = self.defaults["max_grad_norm"]
        return mg is not None and mg > 0

    def _step_gpu(self, groups):
        lib = _lib.load()
        plan = self._gpu_plan(groups, lamb=True)
        stream = torch.cuda.current_stream(self._device()).cuda_stream
        clip = self._clip()
        if clip:
            self._grad_norm(plan, 2, self.defaults["max_grad_norm"], stream)
        elif self.capturable:
            self._step_inc(plan, stream)
        coef = plan["scal"][1:].data_ptr() if clip else None
        T = plan["T"]
        tsum_p, tsum_u = plan["tsum"][T:2 * T], plan["tsum"][2 * T:]
        nch = plan["nch"]
        part_p, part_u = plan["partials"][:nch], plan["partials"][nch:]
        args = []
        for gp in plan["groups"]:
            g = gp["group"]
            aux = gp["slots"] if self.capturable else self._host_steps([(None, p, None) for p in gp["params"]])
            lr, lr_dev = self._lr(g)
            b1, b2 = g["betas"]
            wd = float(g["weight_decay"])
            o = gp["off"]
            a = [gp["T"], gp["pgmv"], gp["n"], aux, _ptr(self._steps), lr, lr_dev, float(b1), float(b2),
                 (1.0 - float(b1)) if g["grad_averaging"] else 1.0, float(g["eps"]), wd, int(self.adam_w_mode),
                 int(bool(g["bias_correction"])), int(self.use_nvlamb or wd != 0.0), coef]
            ch0 = sum(lib.mk_mt_chunks(n) for n in list(plan["n"])[:o])
            ws = [part_p[ch0:].data_ptr(), part_u[ch0:].data_ptr(), tsum_p[o:].data_ptr(), tsum_u[o:].data_ptr()]
            _lib.check(lib.mk_mt_lamb(1, *a, *ws, stream), "mk_mt_lamb stage 1")
            args.append((a, ws))
        if plan["red"]:
            plan["red"](tsum_p, tsum_u)
        for a, ws in args:
            _lib.check(lib.mk_mt_lamb(2, *a, *ws, stream), "mk_mt_lamb stage 2")

    def _step_cpu(self, groups):
        gdiv = 1.0
        if self._clip():
            G = self._cpu_norm(groups)
            mg = float(self.defaults["max_grad_norm"])
            gdiv = G / mg if G > mg else 1.0
        ps = [p for _, items in groups for _, p, _ in items]
        us, pn2 = [], []
        for g, items in groups:
            (b1, b2), eps, wd = g["betas"], g["eps"], float(g["weight_decay"])
            b3 = 1.0 - b1 if g["grad_averaging"] else 1.0
            for (_, p, gr), step in zip(items, self._cpu_steps(items)):
                st = self.state[p]
                pr, m, v = _real(p.data), _real(st["m"]), _real(st["v"])
                gv = _real(gr) / gdiv
                if not self.adam_w_mode:
                    gv = gv + wd * pr
                m.mul_(b1).add_(gv, alpha=b3)
                v.mul_(b2).addcmul_(gv, gv, value=1.0 - b2)
                bc1, bc2 = (1.0 - b1 ** step, 1.0 - b2 ** step) if g["bias_correction"] else (1.0, 1.0)
                u = (m / bc1) / ((v / bc2).sqrt() + eps)
                if self.adam_w_mode:
                    u = u + wd * pr
                us.append(u)
                pn2.append(pr)
        tp, tu = _sumsq_cpu(pn2), _sumsq_cpu(us)
        red = _reducer_for(ps, torch.device("cpu"), self._reducers)
        if red:
            red(tp, tu)
        k = 0
        for g, items in groups:
            lr, wd = float(g["lr"]), float(g["weight_decay"])
            for _, p, _ in items:
                pn, un = math.sqrt(tp[k]), math.sqrt(tu[k])
                ratio = lr * (pn / un) if (self.use_nvlamb or wd != 0.0) and pn != 0.0 and un != 0.0 else lr
                _real(p.data).sub_(us[k], alpha=ratio)
                k += 1
