"""Buffers for the guard tests of the streaming kernels (a plain module, imported by test_metrics_guard_gpu.py,
test_preproc_guard_gpu.py, test_specnorm_guard_gpu.py and test_zenith_guard_gpu.py; not a conftest): inputs and outputs that start
a chosen number of elements past a 16-byte boundary, on top of ``guarded`` / ``poisoned`` of tests/kernel_checks.py."""
import torch

from kernel_checks import SENTINEL, guarded, poisoned

_KIND = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    """The bit patterns of a real or complex tensor, as integers of the width of a (real) element."""
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(_KIND[t.element_size()])


def put(t, off, dev):
    """The host tensor ``t`` on the device ``off`` elements past a 16-byte boundary between NaN bands, NaNs in front of an offset
    view; returns (view, whole buffer view, its host input) for ``unchanged`` after the launch."""
    flat = torch.cat([torch.full((off,), float("nan"), dtype=t.dtype), t.reshape(-1)])
    whole = poisoned(flat, dev)
    view = whole[off:].view(t.shape)
    assert view.data_ptr() % 16 == (off * t.element_size()) % 16
    return view, whole, flat


def unchanged(whole, flat, what):
    assert torch.equal(bits(whole.cpu()), bits(flat)), f"{what}: a read-only input was written"


def out_at(shape, dtype, off, dev):
    """A guarded output of ``shape`` that starts ``off`` elements past a 16-byte boundary, the elements in front of it holding the
    sentinel; returns (view, check) with ``check(what)`` asserting the bands and those elements."""
    n = 1
    for s in shape:
        n *= int(s)
    buf, band = guarded((n + off,), dtype, dev)
    view = buf[off:].view(shape)
    assert view.data_ptr() % 16 == (off * buf.element_size()) % 16
    want = bits(torch.full((off,), SENTINEL, dtype=dtype))

    def check(what=""):
        band(what)
        assert torch.equal(bits(buf[:off].cpu()), want), f"{what}: the elements in front of the offset output were written"

    return view, check


def code(dtype):
    """The dtype code of the C ABI: 0 = fp32, 1 = bf16."""
    return {torch.float32: 0, torch.bfloat16: 1}[dtype]


def stream():
    return torch.cuda.current_stream().cuda_stream
