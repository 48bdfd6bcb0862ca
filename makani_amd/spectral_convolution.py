"""SpectralConv / FactorizedSpectralConv on MI355X.

Mirrors ``makani/models/common/spectral_convolution.py:43-265``: same constructor
arguments, ``weight`` shape / init / ``is_shared_mp`` / ``sharded_dims_mp`` annotations,
``forward(x) -> (x, residual)`` with the cast / autocast-off structure of lines 124-148.

When both transforms are this package's HIP transforms and ``operator_type="dhconv"``
the layer runs fused on the private channels-last spectrum: FFT -> Legendre (MFMA)
-> dhconv (MFMA) -> Legendre -> FFT, five to seven launches, no layout round trip and no
``.contiguous()`` copies.  The planar pair (``RealFFT2`` / ``InverseRealFFT2`` on their HIP path) runs the
same way: FFT -> latitude DFT (MFMA) -> dhconv (dense: no triangle) -> latitude DFT -> FFT.  Any other
duck-typed transform pair takes the generic path through ``get_contract_fun``.  ``operator_type="diagonal"`` takes the
generic path too unless ``MK_SPEC_DIAG=fused``: then it runs on the same fused path with ``ops.spec_diag`` (``mk_spec_diag_*``,
the weight ``[in, out, l, m]`` as stored) in place of dhconv.

The dhconv weight keeps the reference's logical shape ``[in, out, l]`` (state-dict
parity) but is *stored* ``[l, in, out]`` (a permuted view), so each degree's
``in x out`` matrix is one contiguous 1.18 MB panel for the per-degree GEMM.
"""
import math

import torch
import torch.nn as nn

from . import comm, ops
from .contractions import get_contract_fun
from .distributed import DistributedInverseRealFFT2, DistributedInverseRealSHT, DistributedRealSHT
from .layers import InverseRealFFT2, RealFFT2
from .sht import InverseRealSHT, RealSHT


def _is_hip_pair(fwd, inv):
    return isinstance(fwd, (RealSHT, DistributedRealSHT)) and isinstance(inv, (InverseRealSHT, DistributedInverseRealSHT))


class SpectralConv(nn.Module):
    def __init__(self, forward_transform, inverse_transform, in_channels, out_channels, operator_type="diagonal",
                 separable=False, bias=False, gain=1.0):
        super().__init__()
        self.forward_transform = forward_transform
        self.inverse_transform = inverse_transform
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.modes_lat = self.inverse_transform.lmax
        self.modes_lon = self.inverse_transform.mmax
        self.scale_residual = (self.forward_transform.nlat != self.inverse_transform.nlat) or \
                              (self.forward_transform.nlon != self.inverse_transform.nlon)
        if hasattr(self.forward_transform, "grid"):
            self.scale_residual = self.scale_residual or (self.forward_transform.grid != self.inverse_transform.grid)
        self.operator_type = operator_type
        self.separable = separable
        assert self.inverse_transform.lmax == self.modes_lat
        assert self.inverse_transform.mmax == self.modes_lon

        weight_shape = [in_channels]
        if not self.separable:
            weight_shape += [out_channels]

        # spectral_convolution.py:59-75: a distributed transform (SHT or planar FFT) exposes its shard shapes
        self._distributed = isinstance(self.inverse_transform, (DistributedInverseRealSHT, DistributedInverseRealFFT2))
        if self._distributed:
            hr, wr = comm.get_rank("h"), comm.get_rank("w")
            self.modes_lat_local = self.inverse_transform.l_shapes[hr]
            self.modes_lon_local = self.inverse_transform.m_shapes[wr]
            self.nlat_local = self.inverse_transform.lat_shapes[hr]
            self.nlon_local = self.inverse_transform.lon_shapes[wr]
            self.l_off = sum(self.inverse_transform.l_shapes[:hr])
            self.m_off = sum(self.inverse_transform.m_shapes[:wr])
        else:
            self.modes_lat_local = self.modes_lat
            self.modes_lon_local = self.modes_lon
            self.nlat_local = self.inverse_transform.nlat
            self.nlon_local = self.inverse_transform.nlon
            self.l_off, self.m_off = 0, 0

        if self.operator_type == "diagonal":
            weight_shape += [self.modes_lat_local, self.modes_lon_local]
        elif self.operator_type == "dhconv":
            weight_shape += [self.modes_lat_local]
        else:
            raise ValueError(f"Unsupported operator type f{self.operator_type}")

        # same initialisation as spectral_convolution.py:98-101 (note: the scale vector has one entry per
        # degree l and multiplies the LAST axis, which for "diagonal" is m -- a reference quirk that only
        # broadcasts when modes_lat == modes_lon; kept as is)
        scale = math.sqrt(gain / in_channels) * torch.ones(self.modes_lat_local, dtype=torch.complex64)
        scale[0] *= math.sqrt(2.0)
        init = scale * torch.randn(*weight_shape, dtype=torch.complex64)
        if self.operator_type == "dhconv" and not self.separable:
            # logical [in, out, l], physical [l, in, out]
            phys = init.permute(2, 0, 1).contiguous()
            self.weight = nn.Parameter(phys.permute(1, 2, 0))
        else:
            self.weight = nn.Parameter(init)

        if self.operator_type == "dhconv":
            self.weight.is_shared_mp = ["matmul", "w"]
            self.weight.sharded_dims_mp = [None for _ in weight_shape]
            self.weight.sharded_dims_mp[-1] = "h"
        else:
            self.weight.is_shared_mp = ["matmul"]
            self.weight.sharded_dims_mp = [None for _ in weight_shape]
            self.weight.sharded_dims_mp[-1] = "w"
            self.weight.sharded_dims_mp[-2] = "h"

        self._contract = get_contract_fun(self.weight, implementation="factorized", separable=separable,
                                          complex=True, operator_type=operator_type)
        self._fused = _is_hip_pair(forward_transform, inverse_transform) and operator_type == "dhconv" and not separable
        # the planar pair on the same fused path where its HIP transforms apply (decided per call: MK_PLANAR_FFT, the device)
        self._planar = (isinstance(forward_transform, RealFFT2) and isinstance(inverse_transform, InverseRealFFT2)
                        and operator_type == "dhconv" and not separable)
        # the diagonal filter on the same fused path (ops.spec_diag in place of ops.dhconv), decided per call: MK_SPEC_DIAG
        self._diag_pair = None
        if operator_type == "diagonal" and not separable:
            if _is_hip_pair(forward_transform, inverse_transform):
                self._diag_pair = "sht"
            elif isinstance(forward_transform, RealFFT2) and isinstance(inverse_transform, InverseRealFFT2):
                self._diag_pair = "planar"

        if bias == "constant":
            self.bias = nn.Parameter(torch.zeros(1, self.out_channels, 1, 1))
        elif bias == "position":
            self.bias = nn.Parameter(torch.zeros(1, self.out_channels, self.nlat_local, self.nlon_local))
            self.bias.is_shared_mp = ["matmul"]
            self.bias.sharded_dims_mp = [None, None, "h", "w"]

    # -- fused path on the private spectrum -------------------------------------------------
    def _weight_tensor(self):
        return self.weight

    def synthesise(self, c, B, odt):
        """Private spectrum ``[L, M, B * C]`` -> ``[B * C, nlat, nlon]`` rows in ``odt`` through the inverse transform."""
        it = self.inverse_transform
        return it.inverse_packed(c, B, odt) if self._distributed else it.inverse_packed(c, odt)

    def residual_from_spectrum(self, c, B, dtype):
        """The scaled residual of ``forward`` from the spectrum it handed out instead (``spectrum_residual``)."""
        with torch.autocast(device_type="cuda", enabled=False):
            r = self.synthesise(c, B, dtype if dtype in (torch.float32, torch.bfloat16) else torch.float32)
        return r.view(B, -1, r.shape[-2], r.shape[-1]).to(dtype)

    def takes_spectral_mix(self):
        """A bias-free 1x1 convolution next to one of this layer's transforms can be handed over as a channel mix of the
        spectrum (``premix`` / ``spectrum_residual``): the plain class on its fused path only."""
        return type(self) is SpectralConv and self._fused

    def _forward_fused(self, x, dtype, want_row_sums=False, premix=None, spectrum_residual=False):
        B, C = x.shape[0], x.shape[1]
        ft, it = self.forward_transform, self.inverse_transform
        # planar spectrum: every (l, m) entry is data -- a degree offset >= mmax switches the kernel's triangle off
        l_off = self.modes_lon if self._planar else self.l_off
        xin = x if x.dtype in (torch.float32, torch.bfloat16) else x.float()
        c = ft.forward_packed_fields(xin.contiguous())[0]
        if premix is not None:
            # the bias-free convolution in front of this layer commutes with the analysis: sht(W x) = W sht(x)
            c = ops.spec_mix(c, premix.weight, B, self.l_off, self.m_off)
            C = premix.out_channels
        # the inverse FFT writes its rows directly in the layer's activation dtype (fp32, or bf16 under AMP)
        odt = dtype if dtype in (torch.float32, torch.bfloat16) else torch.float32
        residual = x
        if self.scale_residual and spectrum_residual:
            residual = c        # the caller mixes the channels of the spectrum before it synthesises the residual
        elif self.scale_residual:
            r = self.synthesise(c, B, odt)
            residual = r.view(B, C, r.shape[-2], r.shape[-1]).to(dtype)
        if self.operator_type == "diagonal":
            # a weight per (l, m), as the parameter stores it (a shard: the local block); the planar spectrum is dense
            y = ops.spec_diag(c, self._weight_tensor(), B, self.l_off, self.m_off, dense=isinstance(ft, RealFFT2))
        else:
            y = ops.dhconv(c, self._weight_tensor(), B, l_off, self.m_off)
        sums = None
        if want_row_sums:       # the inverse FFT hands over the row statistics of its output (mk_irfft_sums)
            out, sums = it.inverse_packed(y, B, odt, True) if self._distributed else it.inverse_packed(y, odt, True)
        else:
            out = it.inverse_packed(y, B, odt) if self._distributed else it.inverse_packed(y, odt)
        out = out.view(B, self.out_channels, out.shape[-2], out.shape[-1])
        return out, residual, sums

    def _takes_diag_fused(self, x):
        """The diagonal filter stays on the private spectrum: ``MK_SPEC_DIAG=fused`` (validated on every call), one of this
        package's HIP transform pairs for this input, fp32 / bf16 rows on the device, the weight as ``ops.spec_diag`` takes it."""
        if self.operator_type != "diagonal" or not ops.spec_diag_fused():
            return False
        if self._diag_pair is None or not (x.is_cuda and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16)):
            return False
        w = self._weight_tensor()
        if not ops.spec_diag_supported(w, w):
            return False
        if self._diag_pair == "sht":
            return True
        ft = self.forward_transform
        return tuple(x.shape[-2:]) == (ft.nlat, ft.nlon) and ft.hip_ready(x) and self.inverse_transform.hip_ready(x)

    def forward(self, x, want_row_sums=False, premix=None, spectrum_residual=False):
        """``want_row_sums`` (this package's blocks only): a third result, the fp64 ``[B*C, 2]`` sums / sums of squares of the rows
        of the filtered field for the instance norm behind the filter, or None where the path cannot deliver them.
        ``premix``: a bias-free ``Conv1x1`` the caller left out in front of this layer; it is applied to the spectrum
        (``ops.spec_mix``).  ``spectrum_residual``: where the residual is a synthesis of the input spectrum, return the
        private spectrum in its place (see ``residual_from_spectrum``).  Both only where ``takes_spectral_mix()``."""
        dtype = x.dtype
        residual = x
        sums = None
        if premix is not None or spectrum_residual:
            assert self.takes_spectral_mix() and x.is_cuda and x.dim() == 4 and (premix is None or self.scale_residual)
        ft = self.forward_transform
        # (other dtypes take the generic path below, which casts to fp32 first, as the reference does)
        fused = self._fused or (self._planar and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16)
                                and tuple(x.shape[-2:]) == (ft.nlat, ft.nlon)
                                and ft.hip_ready(x) and self.inverse_transform.hip_ready(x))
        fused = fused or self._takes_diag_fused(x)
        if fused and x.is_cuda and x.dim() == 4:
            with torch.autocast(device_type="cuda", enabled=False):
                x, residual, sums = self._forward_fused(x, dtype, want_row_sums and not hasattr(self, "bias"), premix,
                                                        spectrum_residual)
            if sums is not None and x.dtype != dtype:
                sums = None                         # a cast behind the kernel: the statistics are those of other values
        else:
            x = x.float()
            with torch.autocast(device_type=x.device.type, enabled=False):
                x = self.forward_transform(x).contiguous()
                if self.scale_residual:
                    residual = self.inverse_transform(x)
                    residual = residual.to(dtype)
            xp = self._contract(x, self._weight_tensor(), separable=self.separable, operator_type=self.operator_type)
            x = xp.contiguous()
            with torch.autocast(device_type=x.device.type, enabled=False):
                x = self.inverse_transform(x)
        if hasattr(self, "bias"):
            x = x + self.bias
        x = x.to(dtype=dtype)
        return (x, residual, sums) if want_row_sums else (x, residual)


class _DenseFactorizedWeight(nn.Module):
    """Stand-in for ``tltorch.FactorizedTensor.new(shape, rank, factorization="ComplexDense")``.

    tensorly-torch is not available; the dense ("ComplexDense" / "Dense") factorization is the
    only one built -- it holds one full tensor and ``to_tensor()`` returns it.
    """

    def __init__(self, shape, complex=True):
        super().__init__()
        dtype = torch.complex64 if complex else torch.float32
        self.shape = tuple(shape)
        self.name = "ComplexDense" if complex else "Dense"
        self.tensor = nn.Parameter(torch.empty(*shape, dtype=dtype))

    def normal_(self, mean=0.0, std=1.0):
        with torch.no_grad():
            if self.tensor.is_complex():
                self.tensor.copy_(mean + std * torch.randn(self.shape, dtype=torch.complex64))
            else:
                self.tensor.normal_(mean, std)
        return self

    def to_tensor(self):
        return self.tensor


class FactorizedSpectralConv(SpectralConv):
    """spectral_convolution.py:151-265 for the dense factorization.

    ``weight`` is a factorized-tensor object whose ``to_tensor()`` is reconstructed every call
    and contracted exactly like ``SpectralConv`` (``_contract_dense_reconstruct``,
    factorizations.py:203-209).  CP / Tucker / TT need tensorly-torch and raise.
    """

    def __init__(self, forward_transform, inverse_transform, in_channels, out_channels, operator_type="diagonal",
                 rank=0.2, factorization=None, separable=False, decomposition_kwargs=dict(), bias=False, gain=1.0):
        super().__init__(forward_transform, inverse_transform, in_channels, out_channels, operator_type=operator_type,
                         separable=separable, bias=bias, gain=gain)
        if factorization is None:
            factorization = "ComplexDense"
        complex_weight = factorization[:7].lower() == "complex"
        if factorization.lower() not in ("complexdense", "dense"):
            raise NotImplementedError(f"factorization {factorization} needs tensorly-torch (absent); "
                                      "only the dense factorization is built")
        self.rank = rank
        self.factorization = factorization
        shape = tuple(self.weight.shape)
        ann = (self.weight.is_shared_mp, self.weight.sharded_dims_mp)
        del self.weight
        self.weight = _DenseFactorizedWeight(shape, complex=complex_weight)
        scale = math.sqrt(gain / float(shape[0]))  # spectral_convolution.py:224-225
        self.weight.normal_(mean=0.0, std=scale)
        self.weight.tensor.is_shared_mp, self.weight.tensor.sharded_dims_mp = ann
        self._complex_weight = complex_weight
        self._contract = get_contract_fun(self.weight, implementation="reconstructed", separable=separable,
                                          complex=complex_weight, operator_type=operator_type)
        self._fused = self._fused and complex_weight
        self._planar = self._planar and complex_weight
        self._diag_pair = self._diag_pair if complex_weight else None

    def _weight_tensor(self):
        return self.weight.to_tensor()

    def forward(self, x):
        if self._complex_weight:
            return super().forward(x)
        # real factorized weights act on the view_as_real layout (spectral_convolution.py:250-258)
        dtype = x.dtype
        residual = x
        x = x.float()
        with torch.autocast(device_type=x.device.type, enabled=False):
            x = self.forward_transform(x).contiguous()
            if self.scale_residual:
                residual = self.inverse_transform(x).to(dtype)
        x = torch.view_as_real(x)
        xp = self._contract(x, self.weight, separable=self.separable, operator_type=self.operator_type)
        x = torch.view_as_complex(xp.contiguous())
        with torch.autocast(device_type="cuda" if x.is_cuda else "cpu", enabled=False):
            x = self.inverse_transform(x)
        if hasattr(self, "bias"):
            x = x + self.bias
        return x.to(dtype=dtype), residual


class ComplexReLU(nn.Module):
    """``makani/models/common/activations.py:20-67``: (leaky) ReLU variants for complex tensors; modes ``cartesian``,
    ``modulus`` (learned bias on |z|), ``halfplane`` (learned angle), ``real`` (acts on the real part only)."""

    def __init__(self, negative_slope=0.0, mode="real", bias_shape=None, scale=1.0):
        super().__init__()
        self.mode = mode
        if self.mode in ("modulus", "halfplane"):
            self.bias = nn.Parameter(scale * torch.ones(bias_shape if bias_shape is not None else (1,), dtype=torch.float32))
        else:
            self.bias = 0
        self.negative_slope = negative_slope
        self.act = nn.LeakyReLU(negative_slope=negative_slope)

    def forward(self, z):
        if self.mode == "cartesian":
            return torch.view_as_complex(self.act(torch.view_as_real(z)))
        if self.mode == "modulus":
            zabs = torch.sqrt(torch.square(z.real) + torch.square(z.imag))
            return torch.where(zabs + self.bias > 0, (zabs + self.bias) * z / zabs, 0.0)
        if self.mode == "halfplane":
            angle = torch.angle(z) - self.bias
            return torch.where(torch.logical_and(0.0 <= angle, angle < torch.pi / 2.0), z, self.negative_slope * z)
        if self.mode == "real":
            zr = torch.view_as_real(z)
            return torch.view_as_complex(torch.stack([self.act(zr[..., 0]), zr[..., 1]], dim=-1))
        raise NotImplementedError


class SpectralAttention(nn.Module):
    """The non-linear filter (``filter_type="non-linear"``; spectral_convolution.py:268-405): forward transform, a small
    complex MLP over the channels of every spectral coefficient (``spectral_layers`` layers with ``ComplexReLU``, then
    ``wout``), inverse transform.  Constructor arguments, parameter names (``w.N``, ``b.N``, ``wout``, ``activations.N.bias``)
    and shapes are the reference's; ``operator_type`` is ``"diagonal"`` (one weight for all modes) or ``"l-dependant"`` (one
    per degree l), anything else raises ``ValueError`` like the reference (so the network default ``"dhconv"`` does).

    Deviation, documented: the reference's ``forward_mlp`` hands the ``view_as_real`` 5-D tensor to a 4-index einsum
    (spectral_convolution.py:367-374 with contractions.py:49-54) and cannot run; the arithmetic here is the evident intent
    -- the same einsums on the complex tensor.  No reference fixture can exist: parity of this class is unpinned.

    With this package's HIP transform pair (``RealSHT`` / ``InverseRealSHT``, their distributed pair, ``RealFFT2`` /
    ``InverseRealFFT2`` on their HIP path), the ``real`` / ``cartesian`` activation, no active dropout and even channel counts
    the layer runs fused on the private channels-last spectrum like ``SpectralConv``: analysis -> ``ops.spec_channel_mlp``
    (one ``mk_spec_cmlp_fwd`` launch per product: bias and ``ComplexReLU`` in the GEMM's epilogue, the triangle only) ->
    synthesis, with no ``spec_unpack`` / ``spec_pack`` and no vendor GEMM.  ``MK_SPEC_ATTN=torch`` (or any other case) takes
    ``_forward_torch``: the public transforms around torch einsums.  Under a distributed pair the ``l-dependant`` weights hold
    the local degrees only (``sharded_dims_mp = ["h", None, None]``); ``diagonal`` weights and the biases are replicated.
    """

    def __init__(self, forward_transform, inverse_transform, in_channels, out_channels, operator_type="diagonal",
                 hidden_size_factor=2, complex_activation="real", bias=False, spectral_layers=1, drop_rate=0.0, gain=1.0):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.operator_type, self.spectral_layers = operator_type, spectral_layers
        self.complex_activation = complex_activation
        self.modes_lat, self.modes_lon = forward_transform.lmax, forward_transform.mmax
        self.forward_transform, self.inverse_transform = forward_transform, inverse_transform
        self.scale_residual = (forward_transform.nlat != inverse_transform.nlat) or (forward_transform.nlon != inverse_transform.nlon)
        if hasattr(forward_transform, "grid"):
            self.scale_residual = self.scale_residual or (forward_transform.grid != inverse_transform.grid)
        assert inverse_transform.lmax == self.modes_lat
        assert inverse_transform.mmax == self.modes_lon
        self._distributed = isinstance(inverse_transform, (DistributedInverseRealSHT, DistributedInverseRealFFT2))
        if self._distributed:
            hr, wr = comm.get_rank("h"), comm.get_rank("w")
            self.modes_lat_local = inverse_transform.l_shapes[hr]
            self.modes_lon_local = inverse_transform.m_shapes[wr]
            self.l_off = sum(inverse_transform.l_shapes[:hr])
            self.m_off = sum(inverse_transform.m_shapes[:wr])
        else:
            self.modes_lat_local, self.modes_lon_local = self.modes_lat, self.modes_lon
            self.l_off, self.m_off = 0, 0
        hidden = int(hidden_size_factor * in_channels)
        self.hidden_channels = hidden
        if operator_type == "diagonal":
            lead = ()
            self._eq = "bixy,io->boxy"
        elif operator_type == "l-dependant":
            lead = (self.modes_lat_local,)
            self._eq = "bixy,xio->boxy"
        else:
            raise ValueError("Unknown operator type")
        w = [math.sqrt(2.0 / in_channels) * torch.randn(*lead, in_channels, hidden, dtype=torch.complex64)]
        for _ in range(1, spectral_layers):
            w.append(math.sqrt(2.0 / hidden) * torch.randn(*lead, hidden, hidden, dtype=torch.complex64))
        self.w = nn.ParameterList([nn.Parameter(t) for t in w])
        scale = math.sqrt(gain / in_channels)
        if bias:
            self.b = nn.ParameterList([nn.Parameter(scale * torch.randn(hidden, 1, 1, dtype=torch.complex64))
                                       for _ in range(spectral_layers)])
        self.wout = nn.Parameter(scale * torch.randn(*lead, hidden, out_channels, dtype=torch.complex64))
        if self._distributed:
            # every rank applies the MLP to its own (l, m) shard: a per-degree weight is a shard along l (and shared over the
            # m shards), a degree-independent weight or a bias is the same on every spatial rank
            for p in list(self.w) + [self.wout]:
                if lead:
                    p.is_shared_mp, p.sharded_dims_mp = ["matmul", "w"], ["h", None, None]
                else:
                    p.is_shared_mp, p.sharded_dims_mp = ["spatial"], [None, None]
            for p in (self.b if bias else ()):
                p.is_shared_mp, p.sharded_dims_mp = ["spatial"], [None, None, None]
        self.activations = nn.ModuleList([ComplexReLU(mode=complex_activation, bias_shape=(hidden, 1, 1), scale=scale)
                                          for _ in range(spectral_layers)])
        self.drop = nn.Dropout(drop_rate) if drop_rate > 0.0 else nn.Identity()
        self._hip_pair = _is_hip_pair(forward_transform, inverse_transform)
        self._planar = isinstance(forward_transform, RealFFT2) and isinstance(inverse_transform, InverseRealFFT2)

    def forward_mlp(self, x):
        for layer in range(self.spectral_layers):
            x = torch.einsum(self._eq, x, self.w[layer])
            if hasattr(self, "b"):
                x = x + self.b[layer]
            x = self.activations[layer](x)
            if not isinstance(self.drop, nn.Identity):
                x = torch.view_as_complex(self.drop(torch.view_as_real(x)))
        return torch.einsum(self._eq, x, self.wout)

    def _takes_fused(self, x):
        """The fused path applies: the kernels' activations and channel counts, no active dropout, the bf16x3 engine, this
        package's HIP transforms for this input, and ``MK_SPEC_ATTN`` not ``torch``."""
        hip = ops.spec_attn_hip()       # validates the knob on every call
        if not (hip and x.is_cuda and x.dim() == 4 and self.complex_activation in ("real", "cartesian")):
            return False
        if self.training and not isinstance(self.drop, nn.Identity):
            return False
        if self.in_channels % 2 or self.hidden_channels % 2 or self.out_channels % 2 or ops.SPECTRAL_GEMM != "bf16x3":
            return False
        if self._hip_pair:
            return True
        ft = self.forward_transform
        return (self._planar and x.dtype in (torch.float32, torch.bfloat16) and tuple(x.shape[-2:]) == (ft.nlat, ft.nlon)
                and ft.hip_ready(x) and self.inverse_transform.hip_ready(x))

    def _forward_fused(self, x, dtype, want_row_sums=False):
        B, C = x.shape[0], x.shape[1]
        ft, it = self.forward_transform, self.inverse_transform
        # planar spectrum: every (l, m) entry is data -- a degree offset >= mmax switches the kernels' triangle off
        l_off = self.modes_lon if self._planar else self.l_off
        xin = x if x.dtype in (torch.float32, torch.bfloat16) else x.float()
        c = ft.forward_packed_fields(xin.contiguous())[0]
        odt = dtype if dtype in (torch.float32, torch.bfloat16) else torch.float32
        residual = x
        if self.scale_residual:
            r = it.inverse_packed(c, B, odt) if self._distributed else it.inverse_packed(c, odt)
            residual = r.view(B, C, r.shape[-2], r.shape[-1]).to(dtype)
        y = ops.spec_channel_mlp(c, list(self.w), list(self.b) if hasattr(self, "b") else None, self.wout, B,
                                 self.complex_activation, self.operator_type == "l-dependant", l_off, self.m_off)
        sums = None
        if want_row_sums and self._distributed:     # the local shares, mk_irfft_sums (the sharded norm all-reduces them)
            out, sums = it.inverse_packed(y, B, odt, True)
        elif want_row_sums and isinstance(it, InverseRealSHT):
            # the inverse FFT hands over the row statistics of its output, float64 in a fixed order like the planar pair's
            # (mk_irfft_sums_ws): they are those of the stored rows to 1e-12 whichever pair the layer was built on
            out, sums = it.inverse_packed(y, odt, True, exact_sums=True)
        elif want_row_sums:
            out, sums = it.inverse_packed(y, odt, True)
        else:
            out = it.inverse_packed(y, B, odt) if self._distributed else it.inverse_packed(y, odt)
        out = out.view(B, self.out_channels, out.shape[-2], out.shape[-1])
        return out, residual, sums

    def _forward_torch(self, x):
        dtype = x.dtype
        residual = x
        x = x.to(torch.float32)
        with torch.autocast(device_type=x.device.type, enabled=False):
            x = self.forward_transform(x)
            if self.scale_residual:
                residual = self.inverse_transform(x).to(dtype)
        x = self.forward_mlp(x)
        with torch.autocast(device_type=x.device.type, enabled=False):
            x = self.inverse_transform(x)
        return x.to(dtype), residual

    def forward(self, x, want_row_sums=False):
        """``want_row_sums`` (this package's blocks only): a third result, the fp64 ``[B*C, 2]`` sums / sums of squares of the rows
        of the filtered field for the instance norm behind the filter, or None where the path cannot deliver them."""
        if self._takes_fused(x):
            dtype = x.dtype
            with torch.autocast(device_type="cuda", enabled=False):
                y, residual, sums = self._forward_fused(x, dtype, want_row_sums)
            if sums is not None and y.dtype != dtype:
                sums = None                         # a cast behind the kernel: the statistics are those of other values
            y = y.to(dtype)
        else:
            (y, residual), sums = self._forward_torch(x), None
        return (y, residual, sums) if want_row_sums else (y, residual)
