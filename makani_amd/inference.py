"""Autoregressive rollout inference: the loop of ``makani/utils/inferencer.py`` (``_autoregressive_inference``,
``_autoregressive_inf_lite``, ``predict`` and the fork's ``RMSE_over_time`` / ``RMSE_over_space`` scores of
``inference_epoch``) on this package's step wrappers, with everything behind the model call in ONE pass.

``Rollout(params, stepper, metrics=None, loss=None)`` takes a ``SingleStepWrapper`` or ``MultiStepWrapper``.  Per step it
calls ``stepper.preprocessor.assemble`` and ``stepper.model`` itself and replaces the wrapper's three torch tail calls
(``history_denormalize``, ``mask_output``, ``add_residual``), the held channels, the metric sums, the squared-error map
and the selection / de-normalisation of the output channels by ``ops.rollout_tail`` (``csrc/rollout.hip`` on CUDA
tensors with ``MK_ROLLOUT=hip``, the same steps as torch ops otherwise).  ``stepper.py``, ``preprocessor.py`` and
``metric.py`` are used as they are: ``MetricsHandler.update`` runs its own epilogue on the first five sums of the pass
(``_update_from_sums``).

Deviations from the reference (a fork with local edits), keeping the evident intent:

* ``inferencer.py:241`` holds channel 20 of sample 0 at its input value (``pred[0, 20] = inpt[0, 20]``).  Here
  ``params.held_channels`` names the channels (a list of predicted-channel indices; absent or empty by default, which is
  upstream behaviour) and they are held for ALL samples, in the scored rollout as well as in the free-running one
  (``held_channels=[20]`` at B = 1 is the fork).
* ``inferencer.py:193-197`` builds ``RMSE_over_time`` / ``RMSE_over_space`` from sample 0 of every batch and divides by
  the number of batches.  Here every sample ``b`` adds to both and ``finalize`` divides by the number of samples; at
  B = 1 the two agree.  The map adds the samples in ascending ``b``.
* ``RMSE_over_time`` is accumulated in float64 from the pass's unweighted sum of squares divided by the GLOBAL grid size
  (the fork takes an fp32 ``mean`` over the field); under spatial parallelism the sums are all-reduced, never the fields.
* ``predict`` multiplies by ``global_stds`` and adds ``global_means`` on the host; here ``output_stats`` does it inside
  the pass, and the result goes to pinned host memory with non-blocking copies and ONE synchronisation at the end of ``run``.
* The ``Inferencer`` itself (a ``Trainer`` subclass with loaders, checkpoints and logging) is not part of this package:
  the caller brings the tensors.

``EnsembleRollout`` runs E perturbed members per initial condition through the same step and scores them per lead time
with ``ensemble.EnsembleScores`` (CRPS, spread, rank histogram); ``Rollout`` itself is unchanged by it.
"""
import torch
import torch.distributed as dist

from . import comm, ops
from .mappings import gather_from_parallel_region
from .distributed import compute_split_shapes
from .ensemble import member_noise, perturb_members
from .stepper import _engine_input_dtype


def _update_from_sums(metrics, sums5, loss, idt):
    """``MetricsHandler.update`` fed with ready ``[B, C, 5]`` float64 sums (already reduced over the spatial group): its own
    epilogue runs unchanged, only the pass over the fields is not made a second time."""
    metrics._global_sums = lambda prediction, target: sums5
    try:
        metrics.update(None, None, loss, idt)
    finally:
        del metrics._global_sums            # the instance attribute: the class's method is back


class Rollout:
    """Autoregressive inference on a step wrapper of this package (see the module docstring).

    ``params``: the trainer's parameter object; read here are ``valid_autoreg_steps``, ``N_out_channels``,
    ``held_channels`` (optional) and the global grid (``img_crop_shape_x/y``, else ``img_shape_x/y``).  ``metrics``: a
    ``MetricsHandler`` with initialised buffers (its climatology and latitude weights feed the pass); ``loss``: a
    callable ``loss(pred, targ, inp)`` such as ``LossHandler``.  ``capture=True`` captures one step (assemble, model,
    tail) into one graph on static buffers and replays it per step; the per-step copies (target, zenith slice, curves)
    run eagerly between replays."""

    def __init__(self, params, stepper, metrics=None, loss=None, capture=False):
        if comm.get_size("matmul") > 1:
            raise NotImplementedError("Rollout: channel (matmul) parallelism is not supported")
        self.stepper = stepper
        self.preprocessor = stepper.preprocessor
        self.model = stepper.model
        self.metrics = metrics
        self.loss = loss
        self.capture = bool(capture)
        self.steps = int(params.valid_autoreg_steps) + 1
        self.n_out = int(params.N_out_channels)
        held = getattr(params, "held_channels", None)
        self.held_channels = sorted(set(int(c) for c in held)) if held is not None else []
        if self.held_channels and not 0 <= self.held_channels[0] <= self.held_channels[-1] < self.n_out:
            raise ValueError(f"held_channels {self.held_channels} out of range for {self.n_out} output channels")
        gh = getattr(params, "img_crop_shape_x", None) or params.img_shape_x
        gw = getattr(params, "img_crop_shape_y", None) or params.img_shape_y
        self.global_shape = (int(gh), int(gw))
        self.spatial_size = comm.get_size("spatial")
        self.RMSE_over_time = None          # [steps, C] float64: sum over samples of mean_hw (pred - targ)^2
        self.RMSE_over_space = None         # [C, H, W] fp32 (this rank's shard): sum over samples and steps of (pred - targ)^2
        self.n_samples = 0
        self.n_scored_steps = 0
        self.last_sums = None
        self._lists = {}                  # (name, device) -> int32 tensor, built once (nothing is uploaded per step)
        self._wrow = {}
        self._emits = {}
        self._graph = None

    # ---------------------------------------------------------------- buffers
    def _ensure_buffers(self, C, H, W, device):
        if self.RMSE_over_space is None or self.RMSE_over_space.device != device:
            self.RMSE_over_time = torch.zeros(self.steps, C, dtype=torch.float64, device=device)
            self.RMSE_over_space = torch.zeros(C, H, W, dtype=torch.float32, device=device)
        elif tuple(self.RMSE_over_space.shape) != (C, H, W):
            raise ValueError(f"Rollout: fields [C, H, W] = {(C, H, W)} after {tuple(self.RMSE_over_space.shape)}; zero_buffers() "
                             "does not change the shape, make a new Rollout")

    def zero_buffers(self):
        """Reset the ``RMSE_over_time`` and ``RMSE_over_space`` accumulators (and their sample / step counts)."""
        with torch.no_grad():
            if self.RMSE_over_space is not None:
                self.RMSE_over_time.fill_(0)
                self.RMSE_over_space.fill_(0)
        self.n_samples = 0
        self.n_scored_steps = 0

    def _list(self, name, chans, device):
        key = (name, str(device))
        if key not in self._lists:
            self._lists[key] = torch.tensor(list(chans), dtype=torch.int32, device=device) if len(chans) else None
        return self._lists[key]

    # ---------------------------------------------------------------- one step
    def _tail_args(self, inpt, C):
        """The arguments of the pass that the preprocessor decides: statistics, mask, residual, held channels."""
        pp = self.preprocessor
        kw = {}
        if pp.history_normalization_mode != "none":
            kw["mean"], kw["std"] = pp.history_mean[:, :C], pp.history_std[:, :C]
        if pp.masked_channels:
            if pp.masked_channels[-1] >= C:
                raise ValueError(f"masked channel {pp.masked_channels[-1]} is out of range for {C} output channels")
            kw["mask"] = pp.static_features[0, -1]
            kw["mask_chans"] = self._list("mask", pp.masked_channels, inpt.device)
        if pp.learn_residual or self.held_channels:
            kw["x_last"] = pp.expand_history(inpt, pp.n_history + 1)[:, -1]       # read in place
        if pp.learn_residual:
            kw["residual"] = True
            if pp.residual_scale is not None:
                kw["scale"] = pp.residual_scale.reshape(-1)
        if self.held_channels:
            kw["hold_chans"] = self._list("hold", self.held_channels, inpt.device)
        return kw

    def _score_weights(self, H, device):
        if self.metrics is not None:
            return self.metrics.clim, self.metrics.wrow
        if device not in self._wrow:
            self._wrow[device] = torch.ones(H, dtype=torch.float32, device=device)
        return None, self._wrow[device]

    def _step(self, inpt, targ, emit):
        """assemble, the model and the tail: ``(pred, sums, emitted)``; updates the map when ``targ`` is given."""
        pp = self.preprocessor
        inpans = pp.assemble(inpt, out_dtype=_engine_input_dtype(self.model, inpt))
        yn = self.model(inpans)
        B, C, H, W = yn.shape
        kw = self._tail_args(inpt, C)
        if targ is not None:
            kw["clim"], kw["wrow"] = self._score_weights(H, yn.device)
            kw["tar"], kw["err_map"] = targ, self.RMSE_over_space
        if emit is not None:
            kw["emit_chans"], kw["emit_scale"], kw["emit_shift"] = emit
        return ops.rollout_tail(yn, **kw)

    def _captured_step(self, inpt, targ, emit):
        """One step through a graph captured on static buffers (captured on the first call, replayed afterwards)."""
        key = (tuple(inpt.shape), inpt.dtype, None if targ is None else tuple(targ.shape),
               None if emit is None else tuple(None if t is None else t.data_ptr() for t in emit),
               torch.is_autocast_enabled(), self.preprocessor.training)
        g = self._graph
        if g is None or g["key"] != key:
            g = {"key": key, "inp": inpt.clone(), "tar": None if targ is None else targ.clone(), "emit": emit}
            keep = None if targ is None else self.RMSE_over_space.clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):              # warm-up off the capture stream
                self._step(g["inp"], g["tar"], emit)
            torch.cuda.current_stream().wait_stream(side)
            if keep is not None:
                self.RMSE_over_space.copy_(keep)       # the warm-up step is not part of the rollout
            g["graph"] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g["graph"]):
                g["out"] = self._step(g["inp"], g["tar"], emit)
            self._graph = g
        g["inp"].copy_(inpt)
        if targ is not None:
            g["tar"].copy_(targ)
        g["graph"].replay()
        return g["out"]

    def _emit_args(self, output_channels, output_stats, device):
        """The pass's ``(emit_chans, emit_scale, emit_shift)`` for ``run``'s ``output_channels`` / ``output_stats``, or None."""
        if output_channels is None:
            if output_stats is not None:
                raise ValueError("Rollout.run: output_stats without output_channels")
            return None
        chans = [int(c) for c in output_channels]
        if not chans or min(chans) < 0 or max(chans) >= self.n_out:
            raise ValueError(f"Rollout.run: output_channels {chans} out of range for {self.n_out} output channels")
        means = stds = None
        if output_stats is not None:
            means, stds = (torch.as_tensor(t, dtype=torch.float32).reshape(-1).cpu() for t in output_stats)
            if means.numel() != len(chans) or stds.numel() != len(chans):
                raise ValueError(f"Rollout.run: output_stats have {means.numel()} means and {stds.numel()} stds for "
                                 f"{len(chans)} output channels")
        # uploaded once per (channels, statistics, device): a captured step keeps reading the same tensors
        key = (tuple(chans), None if means is None else (tuple(means.tolist()), tuple(stds.tolist())), str(device))
        if key not in self._emits:
            self._emits[key] = (torch.tensor(chans, dtype=torch.int32, device=device),
                                None if stds is None else stds.to(device), None if means is None else means.to(device))
        return self._emits[key]

    # ---------------------------------------------------------------- the rollout
    def run(self, inp, tar=None, steps=None, inp_times=None, tar_times=None, output_channels=None, output_stats=None):
        """One rollout from the initial condition ``inp`` (``[B, T, C, H, W]`` or flattened ``[B, T * C, H, W]``).

        With ``tar`` ``[B, steps, C, H, W]`` it is ``_autoregressive_inference``: per step the loss (if any),
        ``metrics.update(pred, targ, loss, idt)`` (if any) from the pass's sums, ``RMSE_over_time`` / ``RMSE_over_space``,
        then ``append_history``.  Without ``tar`` it is ``_autoregressive_inf_lite``: ``steps`` free-running steps
        (default ``valid_autoreg_steps + 1``).  ``params.held_channels`` are held at their input value in both.

        ``inp_times`` / ``tar_times`` go through ``Preprocessor2D.cache_unpredicted_times`` first (without them the
        unpredicted channels are whatever the caller cached); ``append_history`` rolls them per step.

        ``output_channels`` (a list, repeats allowed) selects what is returned: fp32 ``[steps, B, K, H, W]`` on the host
        (pinned for CUDA inputs), each step copied without blocking, one synchronisation at the end.  ``output_stats =
        (means, stds)`` with K elements each (in the order of ``output_channels``) de-normalises inside the pass,
        ``pred[:, k] * stds[k] + means[k]``; without it the channels come out as they are.  Returns that tensor, or None."""
        pp = self.preprocessor
        if inp_times is not None or tar_times is not None:
            pp.cache_unpredicted_times(inp_times, tar_times, device=inp.device)
        with torch.no_grad():
            inpt = pp.flatten_history(inp)
            device = inpt.device
            scored = tar is not None
            if scored:
                if tar.dim() != 5 or tar.shape[0] != inpt.shape[0]:
                    raise ValueError(f"Rollout.run: target {tuple(tar.shape)} must be [B, steps, C, H, W] with B = {inpt.shape[0]}")
                nsteps = tar.shape[1]
                if nsteps > self.steps:
                    raise ValueError(f"Rollout.run: {nsteps} target steps, valid_autoreg_steps + 1 = {self.steps}")
                self._ensure_buffers(tar.shape[2], tar.shape[3], tar.shape[4], device)
            else:
                nsteps = int(steps) if steps is not None else self.steps
            out = None
            emit = self._emit_args(output_channels, output_stats, device)
            n_global = float(self.global_shape[0] * self.global_shape[1])
            for idt in range(nsteps):
                targ = tar[:, idt] if scored else None
                if self.capture and device.type == "cuda":
                    pred, sums, emitted = self._captured_step(inpt, targ, emit)
                else:
                    pred, sums, emitted = self._step(inpt, targ, emit)
                if scored:
                    if self.spatial_size > 1:
                        dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=comm.get_group("spatial"))
                    self.last_sums = sums          # [B, C, 6] float64 of the whole field (ops.ROLLOUT_SUMS), this step's
                    loss = self.loss(pred, targ, inpt) if self.loss is not None else torch.zeros((), device=device)
                    if self.metrics is not None:
                        _update_from_sums(self.metrics, sums[..., :5], loss, idt)
                    self.RMSE_over_time[idt] += sums[..., 5].sum(dim=0) / n_global
                if emitted is not None:
                    if out is None:
                        out = torch.empty((nsteps,) + tuple(emitted.shape), dtype=torch.float32, pin_memory=device.type == "cuda")
                    out[idt].copy_(emitted, non_blocking=True)
                inpt = pp.append_history(inpt, pred, idt)
            if scored:
                self.n_samples += inpt.shape[0]
                self.n_scored_steps = max(self.n_scored_steps, nsteps)
            if device.type == "cuda":
                torch.cuda.current_stream(device).synchronize()         # once, for the host copies
        return out

    def finalize(self, stds=None, gather=False):
        """``(RMSE_over_time [steps, C], RMSE_over_space [C, H, W])`` fp32 by ``inference_epoch``'s formulas: the curve
        divided by the samples, the map by the samples and the steps, then ``sqrt``, then (``stds`` ``[C]`` given) times
        the standard deviations.  The samples count EVERY ``b`` of every scored ``run`` (the fork scores sample 0 of each
        batch and counts batches).  Data-parallel ranks all-reduce the curve, the map and the count here; spatial ranks
        keep their own shard of the map unless ``gather``.  The accumulators are left as they are."""
        if self.RMSE_over_space is None:
            raise RuntimeError("Rollout.finalize: no scored run yet")
        with torch.no_grad():
            curve, space = self.RMSE_over_time.clone(), self.RMSE_over_space.clone()
            n = torch.tensor(float(self.n_samples), dtype=torch.float64, device=curve.device)
            if dist.is_initialized() and comm.get_size("data") > 1:
                grp = comm.get_group("data")
                for t in (curve, space, n):
                    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=grp)
            curve = torch.sqrt(curve / n).float()
            space = torch.sqrt(space / float(max(self.n_scored_steps, 1)) / n.float())
            if gather and self.spatial_size > 1:
                hs = compute_split_shapes(self.global_shape[0], comm.get_size("h"))
                ws = compute_split_shapes(self.global_shape[1], comm.get_size("w"))
                space = gather_from_parallel_region(gather_from_parallel_region(space, -2, hs, "h"), -1, ws, "w")
            if stds is not None:
                stds = torch.as_tensor(stds, dtype=torch.float32).reshape(-1).to(curve.device)
                curve = curve * stds[None, :]
                space = space * stds[:, None, None]
        return curve, space


class EnsembleRollout(Rollout):
    """An ensemble of ``members`` perturbed rollouts per initial condition, scored by an ``ensemble.EnsembleScores``.

    ``run`` repeats each of the B initial conditions E = ``members`` times (member fastest, so the model runs at batch
    B * E and sample b's members are rows b E ... b E + E - 1), adds ``noise_std * N(0, 1)`` (``torch.randn`` with ``run``'s
    ``generator``; ``noise_std`` defaults to ``params.noise_std``, else 0) to the predicted channels of every history step of
    members 1 ... E - 1 -- member 0 is the unperturbed control -- and steps with ``Rollout``'s own assemble, model and tail.
    Per step the tail's prediction, viewed as ``[B, E, C, H, W]``, goes to ``scores.update(pred, tar[:, idt], idt)``: one
    ``ops.ensemble_sums`` pass, no field is copied.  With ``capture=True`` the step graph is ``Rollout``'s and the scoring
    launch follows the replay on the same stream.  ``Rollout``'s deterministic scores (``metrics``, ``loss``, the RMSE
    accumulators) are not kept here: they are scores of ONE forecast.

    ``noise`` (a ``noise.SphericalNoise`` on the model grid) replaces the white initial perturbation by ``noise_std`` times a
    correlated field per member, history step and channel (``perturb_members``).  With ``step_noise_std > 0`` the state fed back
    after every step is ``pred + step_noise_std * noise.sample(...)`` for members 1 ... E - 1 (``feedback``): a stochastic forcing,
    correlated from step to step where the module's ``phi > 0``; the scored and emitted ``pred`` stays as the tail wrote it.
    Both run outside the captured step graph, like the initial perturbation.

    The unpredicted channels: ``inp_times`` / ``tar_times`` are repeated per member before they are cached; fields that
    the caller cached for B samples are replaced by their per-member repeats."""

    def __init__(self, params, stepper, scores, members, noise_std=None, capture=False, noise=None, step_noise_std=0.0):
        super().__init__(params, stepper, metrics=None, loss=None, capture=capture)
        self.members = int(members)
        if self.members < 1:
            raise ValueError(f"EnsembleRollout: members must be at least 1, got {members}")
        if scores is not None and scores.members != self.members:
            raise ValueError(f"EnsembleRollout: {self.members} members, the scores were built for {scores.members}")
        self.scores = scores
        self.noise_std = float(getattr(params, "noise_std", 0.0) or 0.0) if noise_std is None else float(noise_std)
        self.noise, self.step_noise_std = noise, float(step_noise_std)
        self.last_products = None           # [steps, B, K, Cs, H, W] on the host: the latest run's ``products``
        if self.step_noise_std < 0.0:
            raise ValueError(f"EnsembleRollout: step_noise_std must not be negative, got {step_noise_std}")
        if self.step_noise_std > 0.0 and noise is None:
            raise ValueError("EnsembleRollout: step_noise_std needs a noise module (noise.SphericalNoise)")

    def _repeat_times(self, times):
        if times is None:
            return None
        if torch.is_tensor(times):
            return (times if times.dim() == 3 else times[None]).repeat_interleave(self.members, dim=0)
        import numpy as np
        return np.repeat(np.atleast_2d(np.asarray(times)), self.members, axis=0)

    def perturb(self, inp, generator=None):
        """``[B * E, T * C, H, W]``: each initial condition E times, noise on members 1 ... E - 1 (a new tensor)."""
        return perturb_members(self.preprocessor.flatten_history(inp), self.members, self.noise_std, generator, self.noise)

    def feedback(self, pred):
        """The state the next step starts from: ``pred`` ``[B * E, C, H, W]`` itself, or with ``step_noise_std > 0`` a copy with
        ``step_noise_std * noise.sample(...)`` added to members 1 ... E - 1 (rows ordered sample, member - 1, channel, as in
        ``perturb_members``).  ``pred``, which is scored and emitted, is not touched."""
        E = self.members
        if self.step_noise_std == 0.0 or E < 2:
            return pred
        B = pred.shape[0] // E
        fed = pred.clone()
        fed.view((B, E) + tuple(pred.shape[1:]))[:, 1:] += self.step_noise_std * member_noise(
            self.noise, (B,) + tuple(pred.shape[1:]), E, pred.dtype)
        return fed

    def run(self, inp, tar=None, steps=None, generator=None, inp_times=None, tar_times=None, output_channels=None,
            output_stats=None, products=None):
        """One ensemble rollout from ``inp`` (``[B, T, C, H, W]`` or flattened).  With ``tar`` ``[B, steps, C, H, W]`` every
        step is scored (``scores`` must be given); without it the ensemble runs free for ``steps`` steps.
        ``output_channels`` / ``output_stats`` as in ``Rollout.run``; the result is fp32 ``[steps, B, E, K, H, W]`` on the
        host, or None.

        ``products`` (an ``ensemble.EnsembleProducts`` for E members): every step's ``pred``, viewed as ``[B, E, C, H, W]`` without
        a copy, goes through one ``ops.ensemble_products`` launch behind the tail (behind the replay with ``capture=True``, on the
        same stream, as the scores) and its ``[B, K, Cs, H, W]`` is copied without blocking into pinned host memory;
        ``last_products`` is that ``[steps, B, K, Cs, H, W]`` tensor of the module's ``out_dtype`` after the one synchronisation
        at the end (None without ``products``).  What ``run`` returns does not change.  Under spatial parallelism every rank
        holds its shard of the planes: the products are pointwise."""
        pp, E = self.preprocessor, self.members
        if products is not None and products.members != E:
            raise ValueError(f"EnsembleRollout.run: {E} members, the products were built for {products.members}")
        with torch.no_grad():
            x = self.perturb(inp, generator)
            B, device = x.shape[0] // E, x.device
            if inp_times is not None or tar_times is not None:
                pp.cache_unpredicted_times(self._repeat_times(inp_times), self._repeat_times(tar_times), device=device)
            mode = "train" if pp.training else "eval"
            for name in ("unpredicted_inp_" + mode, "unpredicted_tar_" + mode):
                z = getattr(pp, name)
                if z is not None and E > 1 and z.shape[0] == B:
                    setattr(pp, name, z.repeat_interleave(E, dim=0))
            scored = tar is not None
            if scored:
                if self.scores is None:
                    raise ValueError("EnsembleRollout.run: a target needs scores")
                if tar.dim() != 5 or tar.shape[0] != B:
                    raise ValueError(f"EnsembleRollout.run: target {tuple(tar.shape)} must be [B, steps, C, H, W] with B = {B}")
                nsteps = tar.shape[1]
                if nsteps > self.steps:
                    raise ValueError(f"EnsembleRollout.run: {nsteps} target steps, valid_autoreg_steps + 1 = {self.steps}")
            else:
                nsteps = int(steps) if steps is not None else self.steps
            emit = self._emit_args(output_channels, output_stats, device)
            out = planes = None
            for idt in range(nsteps):
                if self.capture and device.type == "cuda":
                    pred, _, emitted = self._captured_step(x, None, emit)
                else:
                    pred, _, emitted = self._step(x, None, emit)
                if scored:
                    self.scores.update(pred.view((B, E) + tuple(pred.shape[1:])), tar[:, idt], idt)
                if emitted is not None:
                    if out is None:
                        out = torch.empty((nsteps, B, E) + tuple(emitted.shape[1:]), dtype=torch.float32,
                                          pin_memory=device.type == "cuda")
                    out[idt].copy_(emitted.view((B, E) + tuple(emitted.shape[1:])), non_blocking=True)
                if products is not None:
                    made = products(pred.view((B, E) + tuple(pred.shape[1:])))
                    if planes is None:
                        planes = torch.empty((nsteps,) + tuple(made.shape), dtype=made.dtype, pin_memory=device.type == "cuda")
                    planes[idt].copy_(made, non_blocking=True)
                x = pp.append_history(x, self.feedback(pred), idt)
            if device.type == "cuda":
                torch.cuda.current_stream(device).synchronize()         # once, for the host copies
        self.last_products = planes
        return out
