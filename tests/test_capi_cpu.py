"""CPU tests of the C-ABI library: it loads, exports every symbol the header declares,
and its host-side float64 precompute agrees with the oracle.  No kernel launches here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import capi_checks as capi

from makani_amd import _lib, ops
from oracle import sht as osht

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "makani_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    names = _declared_symbols()
    assert len(names) >= 16
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/makani_amd.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    assert set(_lib.SIGNATURES) == set(names)
    assert lib.mk_version() >= 100


_I, _F, _LL, _P8 = ctypes.c_int, ctypes.c_float, ctypes.c_longlong, ctypes.c_void_p
PINNED_SIGNATURES = {      # written out by hand from the header: together they use every C type it declares
    "mk_last_error": (ctypes.c_char_p, []),
    "mk_legendre_x3_bytes": (_LL, [_I, _I, _I, _I]),
    "mk_quadrature": (_I, [_I, _I, _P8, _P8]),                                            # double*
    "mk_rfft": (_I, [_P8, _I, _P8, _P8, _I, _I, _I, _I, _F, _F, _F, _P8]),
    "mk_latdft_fwd": (_I, [_P8, _P8, _P8, _I, _I, _LL, _P8]),
    "mk_token_layernorm_fwd": (_I, [_P8, _I, _LL, _P8, _I, _LL, _P8, _P8, _P8, _I, _LL, _P8, _LL, _P8, _I, _LL, _P8, _LL, _LL,
                                    _F, _P8]),
    "mk_token_linear_fwd": (_I, [_P8, _LL, _P8, _LL, _P8, _P8, _LL, _P8, _LL, _P8, _LL, _P8, _LL, _P8, _LL, _P8, _LL, _LL, _I,
                                 _I, _P8]),
    "mk_attn_bwd_dkv": (_I, [_P8] * 8 + [_I] * 5 + [_P8, _F, _P8]),                       # const long long* strides
}


def test_derived_signatures_match_pinned_literals():
    """_lib.SIGNATURES is parsed from the header; these rows pin what the parser makes of each C type the header uses."""
    for name, want in PINNED_SIGNATURES.items():
        assert _lib.SIGNATURES[name] == want, name


def test_signature_parser_refuses_an_unknown_type():
    """A type the parser has no ctypes for raises and names the declaration: it never becomes an int."""
    ok = "/* c */\n#include <x.h>\nint mk_a(const float* x, long long n /* rows */, void* stream);\nlong long mk_b(void);\n"
    assert _lib.parse_signatures(ok) == {"mk_a": (_I, [_P8, _LL, _P8]), "mk_b": (_LL, [])}
    with pytest.raises(ValueError, match=r"unknown parameter type 'size_t'.*mk_c\("):
        _lib.parse_signatures(ok + "int mk_c(const float* x, size_t n);\n")
    with pytest.raises(ValueError, match=r"unknown return type 'unsigned'.*mk_d\("):
        _lib.parse_signatures(ok + "unsigned mk_d(int n);\n")


def test_build_header_list_is_what_the_sources_include():
    """build.HEADERS feeds the source digest behind stale(): a header that a source includes and the list lacks would let an
    edit of it pass unseen and an old library run, a listed header that nothing includes is dead weight.  The list must be
    the set of quoted includes of build.SOURCES, followed through the headers themselves."""
    from makani_amd import build

    def norm(path):
        return os.path.normpath(os.path.relpath(path, build.CSRC))

    seen, todo = set(), [os.path.join(build.CSRC, s) for s in build.SOURCES]
    while todo:
        path = todo.pop()
        for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', open(path).read(), flags=re.M):
            target = os.path.normpath(os.path.join(os.path.dirname(path), inc))
            if norm(target) not in seen:
                seen.add(norm(target))
                todo.append(target)
    assert seen == {norm(os.path.join(build.CSRC, h)) for h in build.HEADERS}
    assert len(build.HEADERS) == len(set(build.HEADERS))


def test_readme_knob_table_is_what_the_code_reads():
    """README's "Environment knobs" names exactly the ``MK_*`` variables that the package, its C sources and bench.py read --
    directly, or by name through ``ops._knob`` / ``ops._hip_or_torch`` -- and every switch of ``ops.KNOBS`` has such a read."""
    readme = open(os.path.join(ROOT, "README.md")).read()
    documented = set(re.findall(r"MK_[A-Z0-9_]*[A-Z0-9]", readme.split("## Environment knobs", 1)[1]))
    files = [os.path.join(ROOT, "bench.py")]
    for sub in ("makani_amd", os.path.join("makani_amd", "csrc")):
        d = os.path.join(ROOT, sub)
        files += [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith((".py", ".hip", ".h", ".cpp"))]
    read = set()
    for path in files:
        read |= set(re.findall(r'(?:getenv\(|os\.environ\.get\(|os\.environ\[|_knob\(|_hip_or_torch\()\s*"(MK_[A-Z0-9_]+)"', open(path).read()))
    assert documented == read, (sorted(documented - read), sorted(read - documented))
    assert set(ops.KNOBS) <= read, sorted(set(ops.KNOBS) - read)


@pytest.mark.parametrize("env", sorted(set(ops.KNOBS) - {"MK_SPECTRAL_GEMM"}))
def test_knob_reader_validates(env, monkeypatch):
    """``ops._knob``: the default where the variable is unset, every allowed value as it is, anything else an error that names
    the variable and its values.  (``MK_SPECTRAL_GEMM`` reaches the code through ``ops.SPECTRAL_GEMM`` and ``_gemm_mode``.)"""
    values = ops.KNOBS[env]
    monkeypatch.delenv(env, raising=False)
    for v in values:
        assert ops._knob(env, v) == v
    for v in values:
        monkeypatch.setenv(env, v)
        assert ops._knob(env, values[0]) == v
    monkeypatch.setenv(env, "bogus")
    with pytest.raises(ValueError, match=re.escape(f"unknown {env} 'bogus' ({' | '.join(values)})")):
        ops._knob(env, values[0])


def test_spectral_gemm_mode_keeps_its_own_message():
    assert ops.KNOBS["MK_SPECTRAL_GEMM"] == ("bf16x3", "f32")
    assert [ops._gemm_mode(m) for m in ops.KNOBS["MK_SPECTRAL_GEMM"]] == ["bf16x3", "f32"]
    with pytest.raises(ValueError, match=re.escape("unknown spectral GEMM mode 'bogus' (bf16x3 | f32)")):
        ops._gemm_mode("bogus")


@pytest.mark.parametrize("grid", ["equiangular", "legendre-gauss"])
@pytest.mark.parametrize("nlat", [2, 3, 33, 240, 721])
def test_quadrature_matches_oracle(grid, nlat):
    t, w = ops.quadrature(grid, nlat)
    to, wo = osht.quadrature(grid, nlat)
    assert np.abs(t - to).max() < 1e-13
    # Newton-on-P_n (C) vs numpy's eigenvalue leggauss: both float64, agree far below fp32 resolution
    assert np.abs(w - wo).max() < 1e-12 and np.abs(w / wo - 1).max() < 1e-8


@pytest.mark.parametrize("grid,nlat,lmax,mmax", [("equiangular", 33, 16, 17), ("legendre-gauss", 32, 32, 33),
                                                 ("equiangular", 721, 240, 241), ("legendre-gauss", 240, 240, 241)])
def test_legendre_table_matches_oracle(grid, nlat, lmax, mmax):
    tq, w = osht.quadrature(grid, nlat)
    ref = osht.precompute_legpoly(mmax, lmax, tq)
    for wq in (False, True):
        tab = ops.legendre_table(grid, nlat, lmax, mmax, wq).numpy()
        assert tab.shape == (mmax, lmax, ops.legendre_kpad(nlat))
        want = (ref * w[None, None, :] if wq else ref).astype(np.float32)
        got = tab[:, :, :nlat]
        # same float64 recursion rounded once to fp32: allow 1 ulp-scale differences from libm
        assert np.abs(got - want).max() <= 2e-7 * max(1.0, np.abs(want).max())
        assert np.all(tab[:, :, nlat:] == 0)
        for m in range(1, mmax):
            assert np.all(got[m, : min(m, lmax)] == 0)


def test_twiddles():
    for n in (16, 480, 1440):
        tw = ops.fft_twiddles(n).numpy().astype(np.float64)
        h = n // 2
        a = tw[: 2 * h].reshape(h, 2)
        b = tw[2 * h:].reshape(h + 1, 2)
        assert np.abs(a[:, 0] + 1j * a[:, 1] - np.exp(-2j * np.pi * np.arange(h) / h)).max() < 1e-7
        assert np.abs(b[:, 0] + 1j * b[:, 1] - np.exp(-2j * np.pi * np.arange(h + 1) / n)).max() < 1e-7


_P = 4096      # a non-null, 16-byte aligned address that is never dereferenced: validation returns before any launch

# entry point -> its arguments behind (bc, nlat, nlon, mmax, scale0, scale_m, scale_h), as names looked up in the case
_FFT_TAILS = {"mk_rfft": (), "mk_rfft_ex": ("xf_layout",), "mk_irfft_ex": ("xf_layout",), "mk_rfft_pm": ("chans", "cpp"),
              "mk_irfft_pm": ("chans", "cpp"), "mk_irfft_sums": ("xf_layout", "chans", "cpp", "rowsums"),
              "mk_irfft_affine_add": ("xf_layout", "z", "affine")}
_FFT_DEFAULTS = dict(a=_P, b=_P, x_dtype=0, tw=_P, bc=48, nlat=4, nlon=480, mmax=33, xf_layout=0, chans=48, cpp=24, rowsums=_P,
                     z=_P, affine=_P)
FFT_REJECTED = [      # entry point, the input it must refuse (everything else valid)
    ("mk_rfft_ex", dict(nlon=481)),
    ("mk_rfft_ex", dict(mmax=242)),
    ("mk_rfft_ex", dict(xf_layout=2)),
    ("mk_rfft_ex", dict(x_dtype=2)),
    ("mk_rfft", dict(a=None)),
    ("mk_irfft_ex", dict(x_dtype=1, nlon=64)),
    ("mk_irfft_ex", dict(mmax=0)),
    ("mk_rfft_pm", dict(cpp=20)),
    ("mk_rfft_pm", dict(nlon=64)),
    ("mk_irfft_pm", dict(bc=50)),
    ("mk_irfft_sums", dict(rowsums=None)),
    ("mk_irfft_sums", dict(nlon=64)),
    ("mk_irfft_sums", dict(xf_layout=1, cpp=20)),
    ("mk_irfft_affine_add", dict(z=None)),
    ("mk_irfft_affine_add", dict(b=_P + 4)),
    ("mk_irfft_affine_add", dict(xf_layout=3)),
    ("mk_irfft_affine_add", dict(bc=1200, nlat=933, mmax=3)),      # (240 * 933 + 1) * 1200 * 8 >= 2^31
]


@pytest.mark.parametrize("name,bad", FFT_REJECTED, ids=[f"{n}-{'-'.join(f'{k}={v}' for k, v in b.items())}" for n, b in FFT_REJECTED])
def test_fft_entry_points_reject_bad_input(name, bad):
    """Every FFT entry point validates before it launches: code 1 (a refused argument, not a launch failure) and a message."""
    lib = _lib.load()
    a = dict(_FFT_DEFAULTS, **bad)
    if name == "mk_irfft_sums" and "cpp" not in bad:
        a.update(chans=0, cpp=0)      # plain Fourier rows unless the case is about the peer-major ones
    head = (a["a"], a["x_dtype"], a["b"]) if name.startswith("mk_rfft") else (a["a"], a["b"], a["x_dtype"])
    args = head + (a["tw"], a["bc"], a["nlat"], a["nlon"], a["mmax"], 1.0, 1.0, 1.0) + tuple(a[k] for k in _FFT_TAILS[name])
    lib.mk_quadrature(7, 10, 0, 0)      # leaves a message of another function behind: the one below must replace it
    assert getattr(lib, name)(*args, None) == 1
    msg = lib.mk_last_error()
    assert msg and b"unknown grid" not in msg


def test_errors_are_loud():
    lib = _lib.load()
    assert lib.mk_quadrature(7, 10, 0, 0) != 0
    assert b"unknown grid" in lib.mk_last_error()
    with pytest.raises(ValueError):
        ops.quadrature("lobatto", 8)
    # CPU tensors never reach a kernel, and there is no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rfft_raw(torch.zeros(1, 4, 8), ops.fft_twiddles(8), 5, 1.0, 1.0, 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# misaligned pointers: refused by the host checks, with the message of the check (tests/capi_checks.py)
# ---------------------------------------------------------------------------------------------------------------------
_A = capi.A
MISALIGNED = [      # entry point, its arguments in front of the stream with one pointer moved off its alignment, the refusal
    ("mk_pce_gemm_ex", (_A, _A + 8, _A) + (None,) * 5 + (0, None, 1, 64, 64, 64), "x and the weight image must be 16-byte aligned"),
    ("mk_pce_gemm_ex", (_A, _A, _A, None, _A, _A + 4, None, None, 0, None, 1, 64, 64, 64), "addend_affine must be 8-byte aligned"),
    ("mk_pce_mlp", (_A, _A, _A, _A + 8, None, None, None, None, None, 0, 1, 64, 128, 64, 64), "fields and the weight image must be 16-byte aligned"),
    ("mk_pce_mlp", (_A, _A, _A, _A, _A + 4, None, None, None, None, 1, 1, 64, 128, 64, 64), "fields and the weight image must be 16-byte aligned"),
    ("mk_conv1x1_wgrad_act", (_A, _A + 8, _A, 1, 64, 64, 64, 1), "gy and x must be 16-byte aligned (the tiles are read as uint4)"),
    ("mk_conv1x1_wgrad", (_A + 4, _A, _A, 1, 64, 64, 64), "gy and x must be 16-byte aligned (the tiles are read as uint4)", "mk_conv1x1_wgrad_act"),
    ("mk_conv1x1_x3", (_A, 8, _A + 8, 16, _A, 16, 4, 8, 16, 1, 0, 0, 0, 0), "operands must be 16-byte aligned", "conv_x3_launch"),
    ("mk_conv1x1_x3", (_A, 16, _A, 16, _A + 4, 8, 4, 8, 16, 1, 0, 0, 0, 2), "operands must be 16-byte aligned", "conv_x3_launch"),
    ("mk_conv1x1_x3_bias_act", (_A + 8, 8, _A, 16, _A, 16, 4, 8, 16, 1, 0, 0, _A, 1), "operands must be 16-byte aligned", "conv_x3_launch"),
    ("mk_spec_mix_fwd", (_A + 8, _A, _A, 4, 5, 1, 2, 4, 0, 0), "operands must be 16-byte aligned", "spec_mix_check"),
    ("mk_spec_mix_dgrad", (_A, _A, _A + 8, 4, 5, 1, 2, 4, 0, 0), "operands must be 16-byte aligned", "spec_mix_check"),
    ("mk_spec_mix_wgrad", (_A, _A + 8, _A, 4, 5, 1, 2, 4, 0, 0), "operands must be 16-byte aligned", "spec_mix_check"),
]


@pytest.mark.parametrize("case", MISALIGNED, ids=capi.case_ids(MISALIGNED))
def test_misaligned_pointer_is_refused_before_any_launch(case):
    capi.assert_refused(*case)
