"""Input preprocessing of the step wrappers: unpredicted channels, history normalisation, static features.

Constructor, buffers (``static_features`` and ``history_normalization_weights``, both non-persistent), method names and
results of ``makani/models/preprocessor.py`` (``Preprocessor2D``, ``get_preprocessor``).  ``params`` is the trainer's
parameter object (attribute access).  The methods of the reference are views, small copies or calls the trainer makes
outside the model and stay torch ops.  ``cache_unpredicted_times`` is an addition: it fills the unpredicted channel
with the cosine of the solar zenith angle computed on the device from sample times (``zenith.py``), where the reference
takes fields from its data loader.

The hot path is one method the reference does not have, ``assemble(inp, out_dtype=None)``: what both wrappers do before
every model call,

    add_static_features(history_normalize(append_unpredicted_features(inp)))

with the statistics of ``history_compute_stats`` computed and stored on the way and the optional channel mask applied.
``_assemble_torch`` is exactly that composition in torch ops (CPU tensors; an input that requires a gradient in a
statistics mode, so that a gradient THROUGH the statistics comes from ordinary autograd and is correct by construction;
the yardstick of the GPU tests).  CUDA tensors otherwise take one HIP pass that reads every source once and writes the
model input -- fp32, or directly the bf16 field of the pixel-column engine -- once (``ops.input_assemble`` /
``mk_input_assemble``, differentiable in the predicted channels through ``mk_input_assemble_bwd``).  The choice follows
from device, dtype and ``requires_grad`` only; there is no environment knob.  An input that is not fp32 (a bf16
prediction under autocast) is read as it is by the HIP pass and taken through ``.float()`` by the torch formulation.

History statistics (modes ``"exponential"`` and ``"mean"``) are formed from raw sums: per (sample, channel)
``S1 = sum_t w_t sum_hw x`` and ``S2 = sum_t w_t sum_hw x^2`` in float64 (``ops.history_sums`` / ``mk_history_sums`` on
the GPU), then ``m = S1 / N`` and ``var = S2 / N - m^2 (2 - sum_t w_t)`` with N the GLOBAL grid size -- the reference's
``sum w (x - m)^2 / N`` expanded (its fp32 weights sum to 1 only to 6e-8, hence the last factor).  Under spatial
parallelism the ``[B, C + Cu, 2]`` sums take ONE all-reduce over ``"spatial"``; the reference does two, on the mean and
then on the variance.

Where the reference (a fork with local edits) cannot be followed literally, the evident intent is kept:

* ``stepper.py:45,60`` multiply channel 20 of sample 0 by the last static channel, in place.  Here ``params.masked_channels``
  (a list of predicted-channel indices; absent or empty by default, which is upstream behaviour) names the channels;
  they are multiplied by the last static channel for ALL samples and every history step, the input side inside the
  assemble pass (``masked_channels=[20]`` at B = 1 is the fork).
* ``history_denormalize`` raises in the fork for the statistics modes (``preprocessor.py:354``); the formula below the
  raise is implemented.
* Mode ``"mean"`` raises ``TypeError`` in the reference's constructor (line 43); here it means uniform weights
  ``1 / (n_history + 1)``.
* Mode ``"timediff"`` indexes dimension 5 of a 5-D tensor (line 272): ``NotImplementedError``.
* ``add_residual`` writes into its input in place (lines 181-183) and for ``n_history > 0`` returns the whole history,
  which breaks ``append_history``.  Here it is out of place and returns the new last step ``[B, C, H, W]``; it equals
  the reference at ``n_history = 0``.
* Grid conversion is opt-in: ``params.lat`` / ``params.lon`` are taken through ``deg2rad`` when
  ``data_grid_type == model_grid_type``; differing grids raise ``NotImplementedError`` unless ``params.allow_grid_conversion`` is
  true, and then the grid features are built from ``grids.GridConverter(...).get_dst_coords()`` as in the reference (the data
  itself is converted by the loader's call of that class, not here).
* ``netCDF4`` / ``h5py`` readers: a path ending in ``.npy`` is read with numpy, any other path imports the reference's
  reader library lazily and raises a clear ``ImportError`` if it is absent.
"""
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

from . import comm, ops
from .grids import GridConverter
from .mappings import copy_to_parallel_region, reduce_from_parallel_region

_STAT_MODES = ("exponential", "mean")


def get_orography(orography_path):
    """Surface geopotential ``[H, W]`` scaled to [0, 1] (conditioning_inputs.py: variable ``Z`` of a netCDF file)."""
    if str(orography_path).endswith(".npy"):
        orography = np.load(orography_path)
    else:
        try:
            from netCDF4 import Dataset
        except ImportError as e:
            raise ImportError(f"reading the orography from {orography_path} needs netCDF4, which is not installed; "
                              "pass a .npy file instead") from e
        with Dataset(orography_path, "r") as f:
            orography = f.variables["Z"][:, :]
    orography = np.asarray(orography)
    return (orography - orography.min()) / (orography.max() - orography.min())


def get_land_mask(land_mask_path):
    """Land-sea mask ``[H, W]`` (conditioning_inputs.py: ``lsm[0]`` of an HDF5 file)."""
    if str(land_mask_path).endswith(".npy"):
        lsm = np.load(land_mask_path)
        return lsm[0] if lsm.ndim == 3 else lsm
    try:
        import h5py
    except ImportError as e:
        raise ImportError(f"reading the land mask from {land_mask_path} needs h5py, which is not installed; "
                          "pass a .npy file instead") from e
    with h5py.File(land_mask_path, "r") as f:
        return f["lsm"][0, :, :]


class Preprocessor2D(nn.Module):
    def __init__(self, params):
        super().__init__()
        self.n_history = params.n_history
        self.history_normalization_mode = params.history_normalization_mode
        nsteps = self.n_history + 1
        if self.history_normalization_mode == "exponential":
            self.history_normalization_decay = params.history_normalization_decay
            # inverse ordering, since the first element is the oldest
            w = torch.exp((-self.history_normalization_decay) * torch.arange(start=self.n_history, end=-1, step=-1, dtype=torch.float32))
            w = torch.reshape(w / torch.sum(w), (1, -1, 1, 1, 1))
        elif self.history_normalization_mode == "mean":
            w = torch.full((1, nsteps, 1, 1, 1), 1.0 / float(nsteps), dtype=torch.float32)
        elif self.history_normalization_mode == "timediff":
            raise NotImplementedError("history_normalization_mode 'timediff' does not run in the reference either "
                                      "(it reduces over dimension 5 of a 5-D tensor)")
        else:
            w = torch.ones(nsteps, dtype=torch.float32)
        self.register_buffer("history_normalization_weights", w, persistent=False)
        self.history_mean = None
        self.history_std = None
        self.history_eps = 1e-6

        # residual normalization
        self.learn_residual = params.target == "residual"
        if self.learn_residual and params.normalize_residual:
            residual_scale = torch.from_numpy(np.load(params.time_diff_stds_path)).to(torch.float32)
            self.register_buffer("residual_scale", residual_scale, persistent=False)
        else:
            self.residual_scale = None

        self.img_shape = [params.img_shape_x, params.img_shape_y]

        # unpredicted input channels
        self.unpredicted_inp_train = None
        self.unpredicted_tar_train = None
        self.unpredicted_inp_eval = None
        self.unpredicted_tar_eval = None
        # the grid of this rank's shard, kept (the constructor keeps no params) for cache_unpredicted_times, which alone
        # builds anything from it
        self._zenith_grid = SimpleNamespace(**{k: getattr(params, k) for k in (
            "lat", "lon", "img_shape_x", "img_shape_y", "img_local_offset_x", "img_local_offset_y", "img_local_shape_x",
            "img_local_shape_y") if hasattr(params, k)})

        # static features, sliced to this rank's shard
        static_features = None
        start_x = params.img_local_offset_x
        end_x = min(start_x + params.img_local_shape_x, params.img_shape_x)
        start_y = params.img_local_offset_y
        end_y = min(start_y + params.img_local_shape_y, params.img_shape_y)

        if params.add_grid:
            if hasattr(params, "lat") and hasattr(params, "lon"):
                tx = torch.deg2rad(torch.tensor(params.lat).to(torch.float32))
                ty = torch.deg2rad(torch.tensor(params.lon).to(torch.float32))
                if params.data_grid_type != params.model_grid_type:
                    if not getattr(params, "allow_grid_conversion", False):
                        raise NotImplementedError(f"grid conversion {params.data_grid_type} -> {params.model_grid_type} "
                                                  "(GridConverter interpolation) is opt-in: set params.allow_grid_conversion = True "
                                                  "and convert the data with makani_amd.grids.GridConverter")
                    tx, ty = GridConverter(params.data_grid_type, params.model_grid_type, tx, ty).get_dst_coords()
                    tx, ty = tx.to(torch.float32), ty.to(torch.float32)
            else:
                tx = torch.linspace(0, 1, params.img_shape_x + 1, dtype=torch.float32)[0:-1]
                ty = torch.linspace(0, 1, params.img_shape_y + 1, dtype=torch.float32)[0:-1]
            x_grid, y_grid = torch.meshgrid(tx, ty, indexing="ij")
            grid = torch.cat([x_grid.unsqueeze(0).unsqueeze(0), y_grid.unsqueeze(0).unsqueeze(0)], dim=1)
            grid = grid[:, :, start_x:end_x, start_y:end_y]
            if params.gridtype == "sinusoidal":
                num_freq = int(params.grid_num_frequencies) if hasattr(params, "grid_num_frequencies") else 1
                # channel order of the reference: (sin x, sin y) of frequency 1, then of frequency 2, ...
                static_features = torch.cat([torch.sin(grid)] + [torch.sin(freq * grid) for freq in range(2, num_freq + 1)], dim=1)
            else:
                static_features = grid

        if params.add_orography:
            oro = torch.tensor(get_orography(params.orography_path), dtype=torch.float32)
            oro = torch.reshape(oro, (1, 1, oro.shape[0], oro.shape[1]))
            eps = 1.0e-6
            oro = (oro - torch.mean(oro)) / (torch.std(oro) + eps)
            oro = oro[:, :, start_x:end_x, start_y:end_y]
            static_features = oro if static_features is None else torch.cat([static_features, oro], dim=1)

        if params.add_landmask:
            lsm = torch.tensor(get_land_mask(params.landmask_path), dtype=torch.long)
            # one-hot encode and move the channels to the front
            lsm = torch.permute(torch.nn.functional.one_hot(lsm), (2, 0, 1)).to(torch.float32)
            lsm = torch.reshape(lsm, (1, lsm.shape[0], lsm.shape[1], lsm.shape[2]))
            lsm = lsm[:, :, start_x:end_x, start_y:end_y]
            static_features = lsm if static_features is None else torch.cat([static_features, lsm], dim=1)

        self.do_add_static_features = False
        if static_features is not None:
            self.do_add_static_features = True
            self.register_buffer("static_features", static_features.contiguous(), persistent=False)

        # channels multiplied by the last static channel (the fork's hard-coded land-sea mask, see the module docstring)
        masked = getattr(params, "masked_channels", None)
        self.masked_channels = sorted(set(int(c) for c in masked)) if masked is not None else []
        if self.masked_channels:
            if not self.do_add_static_features:
                raise ValueError("masked_channels needs static features: the mask is the last static channel")
            if self.masked_channels[0] < 0:
                raise ValueError(f"masked_channels must be non-negative predicted-channel indices, got {self.masked_channels}")
        self._mask_cache = {}       # (channels per step, device) -> (host list, int32 device tensor of output channels)

    # ---------------------------------------------------------------- views and small copies (the reference's methods)
    def flatten_history(self, x):
        if x.dim() == 5:
            b_, t_, c_, h_, w_ = x.shape
            x = torch.reshape(x, (b_, t_ * c_, h_, w_))
        return x

    def expand_history(self, x, nhist):
        if x.dim() == 4:
            b_, ct_, h_, w_ = x.shape
            x = torch.reshape(x, (b_, nhist, ct_ // nhist, h_, w_))
        return x

    def add_residual(self, x, dx):
        """``dx`` for direct learning; for residual learning the new last step ``x[:, -1] + dx * scale`` (out of place)."""
        if self.learn_residual:
            if self.residual_scale is not None:
                dx = dx * self.residual_scale
            x = self.expand_history(x, nhist=self.n_history + 1)
            return x[:, -1, ...] + dx
        return dx

    def add_static_features(self, x):
        if self.do_add_static_features:
            # the static features are replicated for each sample
            static = torch.tile(self.static_features, dims=(x.shape[0], 1, 1, 1))
            x = torch.cat([x, static], dim=1)
        return x

    def remove_static_features(self, x):
        if self.do_add_static_features:
            nfeat = self.static_features.shape[1]
            x = x[:, : x.shape[1] - nfeat, :, :]
        return x

    def _unpredicted(self):
        """(input, target) unpredicted channels of the current mode (training / evaluation)."""
        if self.training:
            return self.unpredicted_inp_train, self.unpredicted_tar_train
        return self.unpredicted_inp_eval, self.unpredicted_tar_eval

    def append_history(self, x1, x2, step):
        # the target's unpredicted features (such as the zenith angle) of this step become the input's of the next
        uinp, utar = self._unpredicted()
        if (utar is not None) and (step < utar.shape[1]):
            ut = utar[:, step:(step + 1), :, :, :]
            if self.n_history == 0:
                uinp.copy_(ut)
            else:
                uinp.copy_(torch.cat([uinp[:, 1:, :, :, :], ut], dim=1))

        if self.n_history > 0:
            x1 = self.expand_history(x1, nhist=self.n_history + 1)
            x2 = self.expand_history(x2, nhist=1)
            res = self.flatten_history(torch.cat([x1[:, 1:, :, :, :], x2], dim=1))
        else:
            res = x2
        return res

    def append_channels(self, x, xc):
        xdim = x.dim()
        x = self.expand_history(x, self.n_history + 1)
        xc = self.expand_history(xc, self.n_history + 1)
        xo = torch.cat([x, xc], dim=2)
        if xdim == 4:
            xo = self.flatten_history(xo)
        return xo

    # ---------------------------------------------------------------- history statistics
    def _set_stats_from_sums(self, sums):
        """``history_mean`` / ``history_std`` ``[B, Cn, 1, 1]`` fp32 from the local raw sums ``[B, Cn, 2]`` float64: one
        all-reduce over the spatial group, then m = S1 / N and var = S2 / N - m^2 (2 - sum w)."""
        if comm.get_size("spatial") > 1:
            sums = reduce_from_parallel_region(sums, "spatial")
        n = float(self.img_shape[0] * self.img_shape[1])
        wsum = self.history_normalization_weights.double().sum()
        m = sums[..., 0] / n
        var = sums[..., 1] / n - m * m * (2.0 - wsum)
        mean = m.float().reshape(m.shape[0], m.shape[1], 1, 1)
        std = torch.sqrt(var).float().reshape(m.shape[0], m.shape[1], 1, 1)
        self.history_mean = copy_to_parallel_region(mean, "spatial")
        self.history_std = copy_to_parallel_region(std, "spatial")

    def history_compute_stats(self, x, use_hip=True):
        """Stores ``history_mean`` and ``history_std`` of ``x`` (``[B, T * Cn, H, W]`` or 5-D).  Differentiable in ``x``:
        the sums of a CUDA tensor come from the HIP pass only when no gradient is asked for (and ``use_hip``)."""
        if self.history_normalization_mode == "none":
            self.history_mean = torch.zeros((1, 1, 1, 1), dtype=torch.float32, device=x.device)
            self.history_std = torch.ones((1, 1, 1, 1), dtype=torch.float32, device=x.device)
            return
        xr = self.expand_history(x, self.n_history + 1)
        wt = self.history_normalization_weights.reshape(-1)
        if use_hip and xr.is_cuda and not (xr.requires_grad and torch.is_grad_enabled()):
            sums = ops.history_sums(xr, None, wt)
        else:
            sums = ops._history_sums_torch(xr, wt)
        self._set_stats_from_sums(sums)

    def history_normalize(self, x, target=False):
        if self.history_normalization_mode == "none":
            return x
        xdim = x.dim()
        if xdim == 5:
            xshape = x.shape
            x = self.flatten_history(x)
        if target:
            # strip off the unpredicted channels
            xn = (x - self.history_mean[:, : x.shape[1], :, :]) / self.history_std[:, : x.shape[1], :, :]
        else:
            # tile to include the history
            hm = torch.tile(self.history_mean, (1, self.n_history + 1, 1, 1))
            hs = torch.tile(self.history_std, (1, self.n_history + 1, 1, 1))
            xn = (x - hm) / hs
        if xdim == 5:
            xn = torch.reshape(xn, xshape)
        return xn

    def history_denormalize(self, xn, target=False):
        if self.history_normalization_mode == "none":
            return xn
        assert self.history_mean is not None
        assert self.history_std is not None
        xndim = xn.dim()
        if xndim == 5:
            xnshape = xn.shape
            xn = self.flatten_history(xn)
        if target:
            x = xn * self.history_std[:, : xn.shape[1], :, :] + self.history_mean[:, : xn.shape[1], :, :]
        else:
            hm = torch.tile(self.history_mean, (1, self.n_history + 1, 1, 1))
            hs = torch.tile(self.history_std, (1, self.n_history + 1, 1, 1))
            x = xn * hs + hm
        if xndim == 5:
            x = torch.reshape(x, xnshape)
        return x

    # ---------------------------------------------------------------- unpredicted channels
    def cache_unpredicted_features(self, x, y, xz=None, yz=None):
        mode = "train" if self.training else "eval"
        for name, z in (("unpredicted_inp_" + mode, xz), ("unpredicted_tar_" + mode, yz)):
            cached = getattr(self, name)
            if (cached is not None) and (z is not None):
                cached.copy_(z)
            else:
                setattr(self, name, z)
        return x, y

    def cache_unpredicted_times(self, inp_times, tar_times=None, exact=False, device=None):
        """``cache_unpredicted_features`` fed with sample times in place of fields: the unpredicted channel is the cosine
        of the solar zenith angle (``zenith.CosZenith`` on this rank's shard of ``params.lat`` / ``params.lon``, or of
        the loaders' default grid), evaluated on the device.

        ``inp_times`` ``[B, n_history + 1]`` and ``tar_times`` ``[B, n_future + 1]`` (``[T]`` means one sample) hold
        tz-aware datetimes or ``numpy.datetime64``, as ``zenith.sample_times`` returns them; ``exact`` is
        ``zenith.solar_ephemeris``'s.  Either may instead be a ready ``[B, T, 4]`` tensor of ephemeris scalars on the
        device: nothing is uploaded then, so inside a captured graph the call re-evaluates the channel from whatever the
        tensor holds at replay.  The device is that of the tensors already cached, else of a tensor argument, else
        ``device``, else of the static features.  The fields go through ``cache_unpredicted_features`` (copied into the
        cached tensors if there are any), which ``append_history`` then rolls as usual."""
        from . import zenith
        uinp, utar = self._unpredicted()
        if device is None:
            known = [t for t in (uinp, utar, inp_times, tar_times, getattr(self, "static_features", None)) if torch.is_tensor(t)]
            device = known[0].device if known else torch.device("cpu")
        device = torch.empty(0, device=device).device               # with its index: "cuda" and "cuda:0" are one key
        built = self.__dict__.setdefault("_cos_zenith", {})         # device -> CosZenith, made here only
        if device not in built:
            built[device] = zenith.CosZenith.from_params(self._zenith_grid).to(device)
        cosz = built[device]

        def field(times):
            if times is None:
                return None
            if not torch.is_tensor(times):
                eph = np.atleast_2d(zenith.solar_ephemeris(times, exact=exact))
                times = torch.from_numpy(eph[None] if eph.ndim == 2 else eph)
            return cosz(times.to(device))

        return self.cache_unpredicted_features(None, None, field(inp_times), field(tar_times))

    def append_unpredicted_features(self, inp):
        uinp, _ = self._unpredicted()
        if uinp is not None:
            inp = self.append_channels(inp, uinp)
        return inp

    def remove_unpredicted_features(self, inp):
        uinp, _ = self._unpredicted()
        if uinp is not None:
            inpf = self.expand_history(inp, nhist=self.n_history + 1)
            inpc = inpf[:, :, : inpf.shape[2] - uinp.shape[2], :, :]
            inp = self.flatten_history(inpc)
        return inp

    # ---------------------------------------------------------------- the channel mask
    def _masked_outputs(self, cn, device=None):
        """Output channels that the mask multiplies: ``t * cn + c`` for every history step t and masked channel c, as a
        host list and (``device`` given) an int32 tensor there, built once per (channels per step, device)."""
        key = (cn, str(device))
        if key not in self._mask_cache:
            if self.masked_channels and self.masked_channels[-1] >= cn:
                raise ValueError(f"masked channel {self.masked_channels[-1]} is out of range for {cn} channels per step")
            chans = [t * cn + c for t in range(self.n_history + 1) for c in self.masked_channels]
            dev = torch.tensor(chans, dtype=torch.int32, device=device) if device is not None else None
            self._mask_cache[key] = (chans, dev)
        return self._mask_cache[key]

    def mask_output(self, y):
        """The output side of the mask: the masked predicted channels of ``y`` ``[B, C, H, W]`` times the last static
        channel, out of place (the fork does it in place on sample 0, stepper.py:60)."""
        if not self.masked_channels:
            return y
        key = ("out", y.shape[1], str(y.device))
        if key not in self._mask_cache:                  # built once: nothing is uploaded on later calls (graph capture)
            if self.masked_channels[-1] >= y.shape[1]:
                raise ValueError(f"masked channel {self.masked_channels[-1]} is out of range for {y.shape[1]} output channels")
            hit = torch.zeros(1, y.shape[1], 1, 1, dtype=torch.bool)
            hit[:, self.masked_channels] = True
            self._mask_cache[key] = (hit.to(y.device), torch.ones((), dtype=torch.float32, device=y.device))
        hit, one = self._mask_cache[key]
        return y * torch.where(hit, self.static_features[:, -1:, :, :], one)

    # ---------------------------------------------------------------- the assembled model input
    def _assemble_torch(self, inp, out_dtype=None):
        """The reference's four calls (and the mask) in torch ops, on any device; differentiable throughout."""
        if inp.dtype != torch.float32:
            inp = inp.float()
        inpa = self.append_unpredicted_features(inp)
        self.history_compute_stats(inpa, use_hip=False)
        inpan = self.history_normalize(inpa, target=False)
        inpans = self.add_static_features(inpan)
        if self.masked_channels:
            cn = self.flatten_history(inpa).shape[1] // (self.n_history + 1)
            chans, _ = self._masked_outputs(cn)
            # the multiplier is the last channel of inpans; taken from the buffer, which the in-place product leaves alone
            inpans[:, chans, :, :] *= self.static_features[:, -1:, :, :]
        if out_dtype is not None and inpans.dtype != out_dtype:
            inpans = inpans.to(out_dtype)
        return inpans

    def _nothing_to_do(self, inp, out_dtype):
        uinp, _ = self._unpredicted()
        return (uinp is None and not self.do_add_static_features and self.history_normalization_mode == "none"
                and not self.masked_channels and (out_dtype is None or out_dtype == inp.dtype))

    def assemble(self, inp, out_dtype=None):
        """``add_static_features(history_normalize(append_unpredicted_features(inp)))`` with the statistics computed and
        stored on the way and the mask applied: ``[B, T (C + Cu) + Cs, H, W]`` in ``out_dtype`` (fp32 by default; bf16
        is the fp32 result rounded to nearest even).

        CUDA tensors take one HIP pass (``ops.input_assemble``), differentiable in ``inp`` with the statistics held
        constant -- so it is used when the mode is ``"none"`` or ``inp`` does not require a gradient.  CPU tensors, and an
        input that requires a gradient in a statistics mode, take ``_assemble_torch``: the gradient through the
        statistics is then ordinary autograd's.  If nothing is to be done the argument is returned and nothing is
        launched."""
        if self._nothing_to_do(inp, out_dtype):
            return inp
        stats = self.history_normalization_mode in _STAT_MODES
        needs_grad = inp.requires_grad and torch.is_grad_enabled()
        if not inp.is_cuda or (stats and needs_grad):
            return self._assemble_torch(inp, out_dtype)
        x = self.expand_history(inp, self.n_history + 1)
        uinp, _ = self._unpredicted()
        cn = x.shape[2] + (uinp.shape[2] if uinp is not None else 0)
        mean = std = None
        if stats:
            self._set_stats_from_sums(ops.history_sums(x, uinp, self.history_normalization_weights.reshape(-1)))
            mean, std = self.history_mean, self.history_std
        elif self.history_mean is None or self.history_mean.device != x.device:
            self.history_compute_stats(x)           # the constants 0 and 1 of mode "none", made once per device
        mask_chans = self._masked_outputs(cn, x.device)[1] if self.masked_channels else None
        stat = self.static_features[0] if self.do_add_static_features else None
        return ops.input_assemble(x, uinp, stat, mean, std, mask_chans, (stat.shape[0] - 1) if stat is not None else -1,
                                  out_dtype if out_dtype is not None else torch.float32)


def get_preprocessor(params):
    return Preprocessor2D(params)
