"""Dataset histograms: ``histograms.h5`` of ``data_process/get_histograms.py`` (``edges [C, nbins + 1]``, ``data [C, nbins]``),
per-channel value counts over the range ``[min, max]`` of each channel.

The reference sweeps the dataset twice: the first sweep finds each channel's min and max (``DatasetStats`` gives exactly
those, ``mins`` / ``maxs``), the second calls ``np.histogram(x_c, bins=nbins, range=(min_c, max_c))`` per channel and batch
and adds the counts up.  ``DatasetHistograms`` is the second sweep: it builds the edges once on the host with
``ops.hist_edges`` (bit-equal to numpy's) and hands every batch ``[T, C, H, W]`` to ``ops.field_hist`` (one HIP pass on a
device tensor with up to 4096 bins and ``MK_HIST=hip``; torch ops otherwise).  The counts are integers defined by the edge
table alone -- bin ``i`` holds ``edges[i] <= x < edges[i + 1]``, the last bin is closed on the right -- so every path, every
batch size and every order of the samples gives the same arrays, and they equal ``np.histogram``'s.

Beyond the reference's two datasets the result carries ``outside [C, 3]``: the points below the first edge, above the last
and the NaNs of each channel, which ``np.histogram`` drops without a word, and the number of samples.  With the data's own
min and max as the range the first two are zero."""
import os

import numpy as np
import torch
import torch.distributed as dist

from . import comm, ops

KEYS = ("edges", "data", "outside", "count")


class DatasetHistograms:
    """Running per-channel histograms of a dataset of ``[C, H, W]`` samples; see the module docstring.

    ``mins`` / ``maxs``: the range per channel, ``[C]`` or anything that reshapes to it (the ``[1, C, 1, 1]`` arrays of
    ``DatasetStats`` among them).  ``edge_dtype``: ``"float32"`` is what numpy picks for fp32 data and Python-float bounds, the
    reference's case; ``"float64"`` what it picks for float64 data.  Under spatial model parallelism ``update`` takes this
    rank's rows and columns and ``shard_reduce`` combines the shards."""

    def __init__(self, num_channels, mins, maxs, nbins=100, edge_dtype="float32"):
        self.C = int(num_channels)
        lo, hi = np.asarray(mins, dtype=np.float64).reshape(-1), np.asarray(maxs, dtype=np.float64).reshape(-1)
        if lo.size != self.C or hi.size != self.C:
            raise ValueError(f"DatasetHistograms: mins ({lo.size}) and maxs ({hi.size}) must hold one value per channel ({self.C})")
        self.edges = ops.hist_edges(lo, hi, nbins, dtype=edge_dtype)          # [C, nbins + 1] in edge_dtype, on the host
        self.nbins = self.edges.shape[1] - 1
        self.device = None
        self.n_time = 0             # samples

    # -- state -------------------------------------------------------------------------------------------------------------
    def _alloc(self, device):
        self.device = torch.device(device)
        self.edges64 = torch.from_numpy(self.edges.astype(np.float64)).to(self.device)       # the widening is exact
        self.counts = torch.zeros(self.C, self.nbins, dtype=torch.int64, device=self.device)
        self.outside = torch.zeros(self.C, 3, dtype=torch.int64, device=self.device)

    @torch.no_grad()
    def update(self, batch):
        """Add a batch ``[T, C, H, W]`` of samples (fp32; on the device the counts should live on).  No host
        synchronisation on the HIP path; after the first call the launch is the same every time, so a call can be
        captured.  The number of samples is kept on the host: capturing a call counts it once, for its first replay; every
        further replay of the graph needs ``count(T)``."""
        if batch.dim() != 4 or batch.shape[1] != self.C or batch.shape[0] < 1:
            raise ValueError(f"DatasetHistograms.update: batch {tuple(batch.shape)} is not [T, {self.C}, H, W]")
        batch = batch.float()
        if self.device is None:
            self._alloc(batch.device)
        elif batch.device != self.device:
            raise ValueError(f"DatasetHistograms.update: batch on {batch.device}, the counts on {self.device}")
        ops.field_hist(batch, self.edges64, self.counts, self.outside)
        return self.count(batch.shape[0])

    def count(self, T):
        """The host side of one ``update`` of ``T`` samples.  ``update`` calls it; a caller that replays a captured ``update``
        calls it once per replay after the first."""
        self.n_time += int(T)
        return self

    @torch.no_grad()
    def merge(self, other):
        """Add the counts of ``other``, which must have the same edges bit for bit."""
        if self.edges.dtype != other.edges.dtype or not np.array_equal(self.edges, other.edges):
            raise ValueError("DatasetHistograms.merge: the accumulators differ in their edges")
        if other.device is None:
            return self
        if self.device is None:
            self._alloc(other.device)
        self.counts += other.counts.to(self.device)
        self.outside += other.outside.to(self.device)
        self.n_time += other.n_time
        return self

    # -- collectives ---------------------------------------------------------------------------------------------------
    def _default_device(self):
        return torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")

    @torch.no_grad()
    def all_reduce(self, group=None):
        """Sum over sample-parallel ranks (each saw its own samples; all were built with the same edges).  Integer sums:
        every rank ends with the same arrays.  Collective; a rank without samples takes part."""
        if not dist.is_initialized() or dist.get_world_size(group) == 1:
            return self
        if self.device is None:
            self._alloc(self._default_device())
        n = torch.tensor([self.n_time], dtype=torch.int64, device=self.device)
        for t in (self.counts, self.outside, n):
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        self.n_time = int(n)
        return self

    @torch.no_grad()
    def shard_reduce(self):
        """Sum over the spatial shards of one model-parallel instance (each saw its own rows and columns of the same
        samples): the counts of a shard are the counts of its slice, so the sum is the whole.  The number of samples is the
        same on every shard and stays.  Collective."""
        if comm.get_size("spatial") == 1:
            return self
        if self.device is None:
            self._alloc(self._default_device())
        grp = comm.get_group("spatial")
        dist.all_reduce(self.counts, op=dist.ReduceOp.SUM, group=grp)
        dist.all_reduce(self.outside, op=dist.ReduceOp.SUM, group=grp)
        return self

    # -- results -----------------------------------------------------------------------------------------------------------
    def finalize(self):
        """``{"edges": [C, nbins + 1] in the edge dtype, "data": [C, nbins] int64, "outside": [C, 3] int64 (below, above,
        NaN), "count": samples}`` as numpy arrays and an int."""
        if self.n_time == 0:
            raise RuntimeError("DatasetHistograms.finalize: no sample was added")
        return {"edges": self.edges.copy(), "data": self.counts.cpu().numpy(), "outside": self.outside.cpu().numpy(),
                "count": int(self.n_time)}

    def save(self, output_dir):
        """Write ``histograms.npz`` (the keys of ``finalize``) into ``output_dir``, and ``histograms.h5`` with the reference's
        datasets ``edges`` and ``data`` when ``h5py`` imports (that branch has not run anywhere h5py is missing: untested).
        Returns the arrays."""
        out = self.finalize()
        os.makedirs(output_dir, exist_ok=True)
        np.savez(os.path.join(output_dir, "histograms.npz"), **out)
        try:
            import h5py
        except ImportError:
            h5py = None
        if h5py is not None:
            with h5py.File(os.path.join(output_dir, "histograms.h5"), "w") as f:
                f["edges"] = out["edges"]
                f["data"] = out["data"]
        return out
