"""The spectral kernels on the bf16x3 engine (csrc/x3_legendre.hip, csrc/x3_latdft.hip, csrc/x3_spectral.hip) and their
fp32-MFMA fallbacks (csrc/gemm.hip) through the C ABI, held to three checks at once (helpers in tests/kernel_checks.py):

* every written element passes ``x3_elementwise`` against a float64 einsum of the same inputs: ``|y - ref| <= c 2^-23 (|A| @ |B|)``
  with ``c`` from the CPU emulation of the engine's arithmetic (tests/test_kernel_checks_cpu.py), never from the kernels;
* every output lies between sentinel bands (``guarded``) that must survive, every entry the contract leaves alone (``l < m`` of
  the triangular kernels) keeps the sentinel bit for bit, and where the contract gives zeros they are exact zeros;
* every streamed input, table and weight lies between NaN bands (``poisoned``) and spectra hold NaN at every ``l < m`` entry, so
  a read past a stager's predicate shows up as a NaN in a checked output.

The shapes are the smallest that reach each edge of the 128 x 128 tile, the 64 x 64 wave sub-tile, the 32-row band and the
32-k step; contraction lengths stay at or below 280, where a single dropped piece product still lies three times over ``c``."""
import math

import pytest
import torch

import kernel_checks as kc

pytestmark = pytest.mark.gpu

NAN = float("nan")
ENGINES = {"x3": kc.X3_C, "f32": kc.F32_C}


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def _gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * 131 ** i for i, s in enumerate(seed)) % (2 ** 31))


def _crand(g, *shape):
    return torch.complex(torch.randn(*shape, generator=g), torch.randn(*shape, generator=g))


def _c128(t):
    return t.to(torch.complex128) if t.is_complex() else t.double()


def _tri(L, M, l_off=0, m_off=0):
    """[L, M] bool: global degree >= global mode."""
    return (l_off + torch.arange(L))[:, None] >= (m_off + torch.arange(M))[None, :]


def _with_nan(t, valid):
    """``t`` with zeros (the reference's copy) and with NaN (the kernel's copy) wherever ``valid`` is false."""
    nan = torch.full((), complex(NAN, NAN) if t.is_complex() else NAN, dtype=t.dtype)
    return torch.where(valid, t, torch.zeros((), dtype=t.dtype)), torch.where(valid, t, nan)


def _spectrum(g, dev, L, M, B, C, l_off, m_off):
    """A private spectrum [L][M][B][C]: (float64 copy with zeros at l < m, device copy between NaN bands with NaN at l < m,
    the [L, M, 1, 1] mask of the valid entries)."""
    valid = _tri(L, M, l_off, m_off)[:, :, None, None]
    clean, nan = _with_nan(_crand(g, L, M, B, C), valid)
    return _c128(clean), kc.poisoned(nan, dev), valid


def _is_sentinel(t):
    """Per element: does it hold the sentinel bit for bit?"""
    if t.is_complex():
        want = torch.view_as_real(torch.tensor([kc.SENTINEL_C], dtype=t.dtype)).view(torch.int32)[0]
        return (torch.view_as_real(t).contiguous().view(torch.int32) == want).all(-1)
    return t.contiguous().view(torch.int32) == int(torch.tensor([kc.SENTINEL], dtype=t.dtype).view(torch.int32))


def _worst_row(y, ref, written):
    rows = written.reshape(-1, written.shape[-1]).all(-1)
    r, g = ref.reshape(-1, ref.shape[-1])[rows], y.reshape(-1, y.shape[-1])[rows]
    keep = (r.abs() ** 2).sum(-1) > 0
    if not bool(keep.any()):
        return 0.0
    return float(kc.row_rel(g[keep].to(r.dtype).numpy(), r[keep].numpy()).max())


def _raw_ratio(y, ref, mag, slack):
    """For the record, where a slack was granted: the worst |y - ref| / (2^-23 mag) before the slack is taken off."""
    if slack is None:
        return ""
    err, unit = (kc._components(y) - kc._components(ref)).abs(), 2.0 ** -23 * kc._components(mag)
    return f" ({float((err[unit > 0] / unit[unit > 0]).max()):.2f} before the slack)"


def _check(name, out, check, ref, mag, written=None, c=kc.X3_C, slack=None):
    """After the launch: bands intact, unwritten entries still the sentinel, written entries none of them the sentinel and all
    inside the criterion (which also refuses NaN); prints the worst ratio and the worst row."""
    torch.cuda.synchronize()
    check(name)
    y = out.detach().cpu()
    written = torch.ones(y.shape, dtype=torch.bool) if written is None else written.expand(y.shape)
    sent = _is_sentinel(y)
    assert bool(sent[~written].all()), f"{name}: {int((~sent[~written]).sum())} entries the contract leaves alone were written"
    assert not bool(sent[written].any()), f"{name}: {int(sent[written].sum())} entries the contract writes still hold the sentinel"
    zero = torch.zeros((), dtype=ref.dtype)
    ref, mag = torch.where(written, ref, zero), torch.where(written, mag, zero)
    slack = None if slack is None else torch.where(written, slack, torch.zeros((), dtype=slack.dtype))
    worst = kc.x3_elementwise(torch.where(written, y, torch.zeros((), dtype=y.dtype)), ref, mag, c=c, slack64=slack, what=name)
    print(f"[x3 guard] {name}: worst ratio {worst:.2f} of {c}{_raw_ratio(y, ref, mag, slack)}, worst row {_worst_row(y, ref, written):.2e}")
    return y


def _untouched(name, out, check):
    torch.cuda.synchronize()
    check(name)
    assert bool(_is_sentinel(out.detach().cpu()).all()), f"{name}: a refused call wrote its output"


def _refused(lib, rc, text):
    assert rc != 0 and text in lib.mk_last_error().decode(), (rc, lib.mk_last_error().decode())


def _workspace(nbytes, dev):
    """A 16-byte-aligned workspace of the queried size whose floats all read as NaN (a partial panel that is read without having
    been written shows up), or None for 0 bytes."""
    if nbytes == 0:
        return None, 0
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 16 == 0
    return ws, ws.data_ptr()


def _relu_parts(t, re, im):
    return torch.complex(torch.relu(t.real) if re else t.real, torch.relu(t.imag) if im else t.imag)


# ---------------------------------------------------------------------------------------------------------------------
# Legendre analysis / synthesis: bf16x3 in both Fourier-row layouts, and the fp32-MFMA kernels
# ---------------------------------------------------------------------------------------------------------------------
# (grid, nlat, lmax, mmax_glob, bc, m_off, mmax_loc)
LEG = [
    (0, 33, 16, 17, 1, 0, 17),       # N2 = 2; K = 33: one past a k-step; mode 16 has no degree (fwd: nothing, inv: zeros)
    (1, 131, 140, 35, 33, 0, 35),    # two row tiles (the second ragged, left early for lmax - m <= 128); two latitude tiles 128 + 3;
                                     # K = 131; N2 = 66: two live columns in the second wave column; modes 32..34 start at k-step 1
    (1, 131, 140, 35, 33, 30, 5),    # the same table, a shard that straddles that k-step boundary and ends at mmax_glob
    (0, 9, 8, 8, 65, 0, 8),          # N2 = 130: two column tiles, the second with two columns
]
LEG_VARIANTS = [("x3", 0), ("x3", 1), ("f32", 0)]


@pytest.fixture(scope="module")
def leg_tables():
    cache = {}

    def get(grid, nlat, lmax, mmax, quad):
        key = (grid, nlat, lmax, mmax, quad)
        if key not in cache:
            from makani_amd import _lib
            lib = _lib.load()
            tab = torch.zeros(mmax, lmax, lib.mk_legendre_kpad(nlat))
            _lib.check(lib.mk_legendre_table(grid, nlat, lmax, mmax, quad, tab.data_ptr()), "mk_legendre_table")
            cache[key] = tab
        return cache[key]

    return get


def _leg_table_operand(lib, dev, engine, tab, nlat, lmax, mmax, inverse):
    """The table as the kernel takes it: the fp32 table between NaN bands, or the tile image mk_legendre_x3_split makes of it."""
    from makani_amd import _lib, ops
    tabd = kc.poisoned(tab, dev)
    if engine == "f32":
        return tabd, tabd
    nbytes = lib.mk_legendre_x3_bytes(nlat, lmax, mmax, inverse)
    assert nbytes > 0 and nbytes % 16 == 0
    img = torch.full((nbytes // 4,), NAN, device=dev)
    _lib.check(lib.mk_legendre_x3_split(tabd.data_ptr(), img.data_ptr(), nlat, lmax, mmax, inverse, ops._stream()), "mk_legendre_x3_split")
    return img, tabd


@pytest.mark.parametrize("engine,layout", LEG_VARIANTS, ids=[f"{e}-layout{k}" for e, k in LEG_VARIANTS])
@pytest.mark.parametrize("grid,nlat,lmax,mmax,bc,m_off,mloc", LEG)
def test_legendre_fwd(dev, leg_tables, grid, nlat, lmax, mmax, bc, m_off, mloc, engine, layout):
    from makani_amd import _lib, ops
    lib = _lib.load()
    case, N2 = (grid, nlat, lmax, mmax, bc, m_off, mloc), 2 * bc
    tab = leg_tables(grid, nlat, lmax, mmax, 1)
    g = _gen(1, *case)
    xf = torch.randn(mloc, nlat, N2, generator=g)                                         # [m][k][n]
    xfd = kc.poisoned(xf.transpose(0, 1).contiguous() if layout else xf, dev)
    tabx, keep = _leg_table_operand(lib, dev, engine, tab, nlat, lmax, mmax, 0)
    t64 = tab[m_off:m_off + mloc, :, :nlat].double()
    ref, mag = torch.einsum("mlk,mkn->lmn", t64, xf.double()), kc.absdot("mlk,mkn->lmn", t64, xf)
    c, check = kc.guarded((lmax, mloc, N2), torch.float32, dev)
    if engine == "x3" and layout:
        rc = lib.mk_legendre_fwd_x3_ex(xfd.data_ptr(), tabx.data_ptr(), c.data_ptr(), bc, nlat, lmax, mloc, m_off, mmax, layout, ops._stream())
    elif engine == "x3":        # the entry point without a layout argument is layout 0
        rc = lib.mk_legendre_fwd_x3(xfd.data_ptr(), tabx.data_ptr(), c.data_ptr(), bc, nlat, lmax, mloc, m_off, mmax, ops._stream())
    else:
        rc = lib.mk_legendre_fwd(xfd.data_ptr(), tabx.data_ptr(), c.data_ptr(), bc, nlat, lmax, mloc, m_off, mmax, ops._stream())
    _lib.check(rc, "legendre fwd")
    written = _tri(lmax, mloc, 0, m_off)[:, :, None]
    _check(f"legendre fwd {engine} layout {layout} {case}", c, check, ref, mag, written, c=ENGINES[engine],
           slack=kc.x3_slack_underflow("mlk,mkn->lmn", t64, xf) if engine == "x3" else None)


@pytest.mark.parametrize("engine,layout", LEG_VARIANTS, ids=[f"{e}-layout{k}" for e, k in LEG_VARIANTS])
@pytest.mark.parametrize("grid,nlat,lmax,mmax,bc,m_off,mloc", LEG)
def test_legendre_inv(dev, leg_tables, grid, nlat, lmax, mmax, bc, m_off, mloc, engine, layout):
    from makani_amd import _lib, ops
    lib = _lib.load()
    case, N2 = (grid, nlat, lmax, mmax, bc, m_off, mloc), 2 * bc
    tab = leg_tables(grid, nlat, lmax, mmax, 0)
    g = _gen(2, *case)
    valid = _tri(lmax, mloc, 0, m_off)[:, :, None]
    cc, cn = _with_nan(torch.randn(lmax, mloc, N2, generator=g), valid)                   # [l][m][n], NaN at l < m
    cd = kc.poisoned(cn, dev)
    tabx, keep = _leg_table_operand(lib, dev, engine, tab, nlat, lmax, mmax, 1)
    t64 = tab[m_off:m_off + mloc, :, :nlat].double()
    ref, mag = torch.einsum("mlk,lmn->mkn", t64, cc.double()), kc.absdot("mlk,lmn->mkn", t64, cc)
    # the table of a high mode falls through the subnormals to zero next to the poles: what the split loses there (bf16x3 only)
    slack = kc.x3_slack_underflow("mlk,lmn->mkn", t64, cc) if engine == "x3" else None
    if layout:
        ref, mag = ref.transpose(0, 1).contiguous(), mag.transpose(0, 1).contiguous()
        slack = None if slack is None else slack.transpose(0, 1).contiguous()
    xf, check = kc.guarded((nlat, mloc, N2) if layout else (mloc, nlat, N2), torch.float32, dev)
    if engine == "x3" and layout:
        rc = lib.mk_legendre_inv_x3_ex(cd.data_ptr(), tabx.data_ptr(), xf.data_ptr(), bc, nlat, lmax, mloc, m_off, mmax, layout, ops._stream())
    elif engine == "x3":
        rc = lib.mk_legendre_inv_x3(cd.data_ptr(), tabx.data_ptr(), xf.data_ptr(), bc, nlat, lmax, mloc, m_off, mmax, ops._stream())
    else:
        rc = lib.mk_legendre_inv(cd.data_ptr(), tabx.data_ptr(), xf.data_ptr(), bc, nlat, lmax, mloc, m_off, mmax, ops._stream())
    _lib.check(rc, "legendre inv")
    y = _check(f"legendre inv {engine} layout {layout} {case}", xf, check, ref, mag, c=ENGINES[engine], slack=slack)
    for m in range(mloc):
        if m_off + m >= lmax:       # a mode without a degree: the synthesis is an exact zero, not the sentinel
            assert bool(((y[:, m] if layout else y[m]) == 0).all()), f"mode {m_off + m} >= lmax must give zeros"


# ---------------------------------------------------------------------------------------------------------------------
# latitude DFT of the planar transform
# ---------------------------------------------------------------------------------------------------------------------
DFT = [(2, 2, 1), (70, 33, 33), (131, 130, 65)]        # (nlat, lmax, ncols)


def _dft_matrix(nlat, lmax):
    """W[l][k] = exp(-2 pi i f_l k / nlat) / sqrt(nlat) in float64, f_l = l for l < ceil(lmax / 2), else nlat - lmax + l (the
    header's formula, the angle reduced modulo nlat in integers)."""
    half = (lmax + 1) // 2
    f = torch.tensor([l if l < half else nlat - lmax + l for l in range(lmax)])
    ang = ((f[:, None] * torch.arange(nlat)[None, :]) % nlat).double() * (-2.0 * math.pi / nlat)
    return torch.complex(torch.cos(ang), torch.sin(ang)) / math.sqrt(nlat)


def _dft_table(lib, dev, nlat, lmax):
    from makani_amd import _lib
    n = lib.mk_latdft_table_len(nlat, lmax)
    assert n == 2 * lmax * ((nlat + 3) // 4 * 4) + 2 * nlat * ((lmax + 3) // 4 * 4)
    tab = torch.zeros(n)
    _lib.check(lib.mk_latdft_table(nlat, lmax, tab.data_ptr()), "mk_latdft_table")
    return kc.poisoned(tab, dev)


@pytest.mark.parametrize("nlat,lmax,ncols", DFT)
def test_latdft(dev, nlat, lmax, ncols):
    """Forward and inverse against the float64 matrix of the header's formula: the table's rounding to fp32 is at most
    2^-24 mag and sits inside c; the epilogue's sum of two accumulators is the slack."""
    from makani_amd import _lib, ops
    lib = _lib.load()
    W = _dft_matrix(nlat, lmax)
    tab = _dft_table(lib, dev, nlat, lmax)
    g = _gen(3, nlat, lmax, ncols)
    xf, cs = _crand(g, nlat, ncols), _crand(g, lmax, ncols)
    xfd, csd = kc.poisoned(xf, dev), kc.poisoned(cs, dev)
    ref, mag = W @ _c128(xf), kc.absdot("lk,kj->lj", W, xf)
    c, check = kc.guarded((lmax, ncols), torch.complex64, dev)
    _lib.check(lib.mk_latdft_fwd(xfd.data_ptr(), tab.data_ptr(), c.data_ptr(), nlat, lmax, ncols, ops._stream()), "mk_latdft_fwd")
    _check(f"latdft fwd {(nlat, lmax, ncols)}", c, check, ref, mag, slack=kc.x3_slack_add(ref))
    ref, mag = W.conj().T @ _c128(cs), kc.absdot("lk,lj->kj", W, cs)
    x, check = kc.guarded((nlat, ncols), torch.complex64, dev)
    _lib.check(lib.mk_latdft_inv(csd.data_ptr(), tab.data_ptr(), x.data_ptr(), nlat, lmax, ncols, ops._stream()), "mk_latdft_inv")
    _check(f"latdft inv {(nlat, lmax, ncols)}", x, check, ref, mag, slack=kc.x3_slack_add(ref))


def test_latdft_refuses_lmax_over_nlat(dev):
    from makani_amd import _lib, ops
    lib = _lib.load()
    tab = _dft_table(lib, dev, 8, 8)
    xf = kc.poisoned(_crand(_gen(4), 9, 4), dev)
    for fn in (lib.mk_latdft_fwd, lib.mk_latdft_inv):
        out, check = kc.guarded((9, 4), torch.complex64, dev)
        _refused(lib, fn(xf.data_ptr(), tab.data_ptr(), out.data_ptr(), 8, 9, 4, ops._stream()), "2 <= lmax <= nlat")
        _untouched("latdft lmax > nlat", out, check)


# ---------------------------------------------------------------------------------------------------------------------
# complex [I][O] panels per degree: dhconv (bf16x3 and fp32 MFMA) and the channel MLP
# ---------------------------------------------------------------------------------------------------------------------
# (L, M, B, I, O, l_off, m_off)
PANEL = [
    (3, 3, 1, 2, 2, 0, 0),
    (130, 131, 1, 6, 34, 0, 0),      # row counts 1..130 cross every band and tile edge; K = 12 < one k-step; 68 floats cross the wave column
    (5, 70, 2, 18, 66, 68, 0),       # dense: 140 rows, ragged second tile; K = 36; 132 floats: two column tiles; the dgrad contracts 132
    (6, 4, 3, 130, 6, 0, 2),         # an m-shard, degrees 0 and 1 without rows; two wgrad row tiles; fwd K = 260, dgrad 260 columns
]
ODD = (16, 17, 2, 7, 5, 0, 0)        # odd channel counts: the fp32 kernels' 8-byte loaders; the bf16x3 kernels refuse
DH = [("x3", s) for s in PANEL] + [("f32", s) for s in PANEL + [ODD]]


def _panel_inputs(dev, seed, L, M, B, I, O, l_off, m_off, per_degree=True):
    g = _gen(seed, L, M, B, I, O, l_off, m_off, per_degree)
    x64, xd, valid = _spectrum(g, dev, L, M, B, I, l_off, m_off)
    gy64, gyd, _ = _spectrum(g, dev, L, M, B, O, l_off, m_off)
    w = _crand(g, L, I, O) if per_degree else _crand(g, I, O)
    return x64, xd, gy64, gyd, _c128(w), kc.poisoned(w, dev), valid


@pytest.mark.parametrize("engine,shape", DH, ids=[f"{e}-{'x'.join(map(str, s))}" for e, s in DH])
def test_dhconv(dev, engine, shape):
    from makani_amd import _lib, ops
    lib = _lib.load()
    L, M, B, I, O, l_off, m_off = shape
    x64, xd, gy64, gyd, w64, wd, valid = _panel_inputs(dev, 5, *shape)
    fn = {k: getattr(lib, f"mk_dhconv_{k}" + ("_x3" if engine == "x3" else "")) for k in ("fwd", "dgrad", "wgrad")}
    c, dims, st = ENGINES[engine], (L, M, B, I, O, l_off, m_off), ops._stream()
    y, check = kc.guarded((L, M, B, O), torch.complex64, dev)
    _lib.check(fn["fwd"](xd.data_ptr(), wd.data_ptr(), y.data_ptr(), *dims, st), "dhconv fwd")
    _check(f"dhconv fwd {engine} {shape}", y, check, torch.einsum("lmbi,lio->lmbo", x64, w64), kc.absdot("lmbi,lio->lmbo", x64, w64), valid, c)
    gx, check = kc.guarded((L, M, B, I), torch.complex64, dev)
    _lib.check(fn["dgrad"](gyd.data_ptr(), wd.data_ptr(), gx.data_ptr(), *dims, st), "dhconv dgrad")
    _check(f"dhconv dgrad {engine} {shape}", gx, check, torch.einsum("lmbo,lio->lmbi", gy64, w64.conj()),
           kc.absdot("lmbo,lio->lmbi", gy64, w64), valid, c)
    gw, check = kc.guarded((L, I, O), torch.complex64, dev)
    _lib.check(fn["wgrad"](xd.data_ptr(), gyd.data_ptr(), gw.data_ptr(), *dims, st), "dhconv wgrad")
    got = _check(f"dhconv wgrad {engine} {shape}", gw, check, torch.einsum("lmbi,lmbo->lio", x64.conj(), gy64),
                 kc.absdot("lmbi,lmbo->lio", x64, gy64), None, c)
    for l in range(L):
        if not bool(valid[l].any()):    # a degree without valid rows: its gradient is an exact zero
            assert bool((got[l] == 0).all()), f"degree {l} has no rows: its weight gradient must be zero"


def test_x3_panels_refuse_odd_channels(dev):
    from makani_amd import _lib, ops
    lib = _lib.load()
    L, M, B, I, O, l_off, m_off = ODD
    x64, xd, gy64, gyd, w64, wd, valid = _panel_inputs(dev, 5, *ODD)
    st = ops._stream()
    for name, a, b, shape in (("fwd", xd, wd, (L, M, B, O)), ("dgrad", gyd, wd, (L, M, B, I)), ("wgrad", xd, gyd, (L, I, O))):
        out, check = kc.guarded(shape, torch.complex64, dev)
        _refused(lib, getattr(lib, f"mk_dhconv_{name}_x3")(a.data_ptr(), b.data_ptr(), out.data_ptr(), *ODD, st), "even channel counts")
        _untouched(f"dhconv {name} x3 odd channels", out, check)
        out, check = kc.guarded(shape, torch.complex64, dev)
        if name == "wgrad":
            rc = lib.mk_spec_cmlp_wgrad(a.data_ptr(), b.data_ptr(), out.data_ptr(), None, *ODD, 1, st)
        else:
            rc = getattr(lib, f"mk_spec_cmlp_{name}")(a.data_ptr(), b.data_ptr(), None, out.data_ptr(), *ODD, 1, 0, st)
        _refused(lib, rc, "even channel counts")
        _untouched(f"cmlp {name} odd channels", out, check)
    # the real channel mix: W [O][I]
    wr = kc.poisoned(torch.randn(O, I, generator=_gen(6)), dev)
    out, check = kc.guarded((L, M, B, O), torch.complex64, dev)
    _refused(lib, lib.mk_spec_mix_fwd(xd.data_ptr(), wr.data_ptr(), out.data_ptr(), *ODD, st), "even channel counts")
    _untouched("mix fwd odd channels", out, check)
    # the block MLP: odd block sizes
    out, check = kc.guarded((L * M * B, O), torch.complex64, dev)
    _refused(lib, lib.mk_spec_bdmlp_fwd(xd.data_ptr(), wd.data_ptr(), out.data_ptr(), L * M * B, 1, I, O, 0, 0.0, st), "even block sizes")
    _untouched("bdmlp fwd odd blocks", out, check)


CMLP = [(s, pd) for s in PANEL for pd in (0, 1)]


@pytest.mark.parametrize("shape,per_degree", CMLP, ids=[f"{'x'.join(map(str, s))}-{'per_degree' if pd else 'shared'}" for s, pd in CMLP])
def test_cmlp_fwd_dgrad(dev, shape, per_degree):
    """Forward with act 0 / 1 / 2, with and without bias (the bias addition is the slack; ReLU needs none); data gradient with
    act 0 / 1 / 2, the mask operand between NaN bands with NaN at l < m."""
    from makani_amd import _lib, ops
    lib = _lib.load()
    L, M, B, I, O, l_off, m_off = shape
    x64, xd, gy64, gyd, w64, wd, valid = _panel_inputs(dev, 7, *shape, per_degree=bool(per_degree))
    g = _gen(8, *shape)
    bias = _crand(g, O)
    biasd = kc.poisoned(bias, dev)
    a64, ad, _ = _spectrum(g, dev, L, M, B, I, l_off, m_off)
    st, eqw = ops._stream(), "lio" if per_degree else "io"
    pre, mag = torch.einsum(f"lmbi,{eqw}->lmbo", x64, w64), kc.absdot(f"lmbi,{eqw}->lmbo", x64, w64)
    for act in (0, 1, 2):
        for b in (None, biasd):
            h = pre if b is None else torch.where(valid, pre + _c128(bias), torch.zeros((), dtype=pre.dtype))
            y, check = kc.guarded((L, M, B, O), torch.complex64, dev)
            _lib.check(lib.mk_spec_cmlp_fwd(xd.data_ptr(), wd.data_ptr(), None if b is None else b.data_ptr(), y.data_ptr(), *shape,
                                            per_degree, act, st), "mk_spec_cmlp_fwd")
            _check(f"cmlp fwd {shape} per_degree={per_degree} act={act} bias={b is not None}", y, check, _relu_parts(h, act >= 1, act == 2),
                   mag, valid, slack=None if b is None else kc.x3_slack_add(h))
    full, mag = torch.einsum(f"lmbo,{eqw}->lmbi", gy64, w64.conj()), kc.absdot(f"lmbo,{eqw}->lmbi", gy64, w64)
    for act in (0, 1, 2):
        mr = (a64.real > 0) if act else torch.ones_like(a64.real, dtype=torch.bool)
        mi = (a64.imag > 0) if act == 2 else torch.ones_like(mr)
        zero = torch.zeros((), dtype=torch.float64)
        ref = torch.complex(torch.where(mr, full.real, zero), torch.where(mi, full.imag, zero))
        gx, check = kc.guarded((L, M, B, I), torch.complex64, dev)
        _lib.check(lib.mk_spec_cmlp_dgrad(gyd.data_ptr(), wd.data_ptr(), ad.data_ptr() if act else None, gx.data_ptr(), *shape,
                                          per_degree, act, st), "mk_spec_cmlp_dgrad")
        _check(f"cmlp dgrad {shape} per_degree={per_degree} act={act}", gx, check, ref, mag, valid)


# the shape of tests/test_specattn_gpu.py::test_shared_weight_gradient_over_several_degree_groups: 2 x 3 tiles, two degrees (of
# different row counts) per workgroup, 100 partial panels
SHARED_WGRAD = PANEL + [(200, 20, 1, 136, 130, 0, 0)]


@pytest.mark.parametrize("shape", SHARED_WGRAD, ids=["x".join(map(str, s)) for s in SHARED_WGRAD])
def test_cmlp_shared_wgrad_and_bgrad(dev, shape):
    """The shared weight gradient (partial panels in the queried workspace, added in a fixed order: the slack is that sum of g
    panels) and the bias gradient (float64 sums, rounded once), each with equal bits on two runs."""
    from makani_amd import _lib, ops
    lib = _lib.load()
    L, M, B, I, O, l_off, m_off = shape
    x64, xd, gy64, gyd, _, _, valid = _panel_inputs(dev, 9, *shape)
    st = ops._stream()
    nbytes = lib.mk_spec_cmlp_wgrad_workspace(L, I, O, 0)
    assert lib.mk_spec_cmlp_wgrad_workspace(L, I, O, 1) == 0 and nbytes % (I * O * 8) == 0
    if shape[0] == 200:
        assert nbytes == 100 * I * O * 8
    groups = max(nbytes // (I * O * 8), 1)
    ref, mag = torch.einsum("lmbi,lmbo->io", x64.conj(), gy64), kc.absdot("lmbi,lmbo->io", x64, gy64)
    runs = []
    for _ in range(2):
        ws, wsp = _workspace(nbytes, dev)
        gw, check = kc.guarded((I, O), torch.complex64, dev)
        _lib.check(lib.mk_spec_cmlp_wgrad(xd.data_ptr(), gyd.data_ptr(), gw.data_ptr(), wsp, *shape, 0, st), "mk_spec_cmlp_wgrad")
        runs.append(_check(f"cmlp shared wgrad {shape} ({groups} panels)", gw, check, ref, mag,
                           slack=kc.x3_slack_sum(groups, mag) if groups > 1 else None))
    assert torch.equal(torch.view_as_real(runs[0]), torch.view_as_real(runs[1])), "the shared weight gradient differs between two runs"
    nbytes = lib.mk_spec_cmlp_bgrad_workspace(L, O)
    assert nbytes == L * O * 16
    ref = gy64.sum(dim=(0, 1, 2))
    mag = torch.complex(gy64.real.abs().sum(dim=(0, 1, 2)), gy64.imag.abs().sum(dim=(0, 1, 2)))
    runs = []
    for _ in range(2):
        ws, wsp = _workspace(nbytes, dev)
        gb, check = kc.guarded((O,), torch.complex64, dev)
        _lib.check(lib.mk_spec_cmlp_bgrad(gyd.data_ptr(), gb.data_ptr(), wsp, L, M, B, O, l_off, m_off, st), "mk_spec_cmlp_bgrad")
        runs.append(_check(f"cmlp bgrad {shape}", gb, check, ref, mag))
    assert torch.equal(torch.view_as_real(runs[0]), torch.view_as_real(runs[1])), "the bias gradient differs between two runs"


@pytest.mark.parametrize("shape", PANEL, ids=["x".join(map(str, s)) for s in PANEL])
def test_cmlp_per_degree_wgrad(dev, shape):
    from makani_amd import _lib, ops
    lib = _lib.load()
    L, M, B, I, O, l_off, m_off = shape
    x64, xd, gy64, gyd, _, _, valid = _panel_inputs(dev, 10, *shape)
    gw, check = kc.guarded((L, I, O), torch.complex64, dev)
    _lib.check(lib.mk_spec_cmlp_wgrad(xd.data_ptr(), gyd.data_ptr(), gw.data_ptr(), None, *shape, 1, ops._stream()), "mk_spec_cmlp_wgrad")
    got = _check(f"cmlp per-degree wgrad {shape}", gw, check, torch.einsum("lmbi,lmbo->lio", x64.conj(), gy64),
                 kc.absdot("lmbi,lmbo->lio", x64, gy64))
    for l in range(L):
        if not bool(valid[l].any()):
            assert bool((got[l] == 0).all()), f"degree {l} has no rows: its weight gradient must be zero"


def test_cmlp_refusals(dev):
    """A mask without a mode, and a misaligned operand; the guarded output stays untouched."""
    from makani_amd import _lib, ops
    lib = _lib.load()
    shape = PANEL[0]
    L, M, B, I, O, l_off, m_off = shape
    x64, xd, gy64, gyd, w64, wd, valid = _panel_inputs(dev, 11, *shape)
    st = ops._stream()
    gx, check = kc.guarded((L, M, B, I), torch.complex64, dev)
    _refused(lib, lib.mk_spec_cmlp_dgrad(gyd.data_ptr(), wd.data_ptr(), xd.data_ptr(), gx.data_ptr(), *shape, 1, 0, st),
             "a mask operand needs an activation mode")
    _untouched("cmlp dgrad mask without a mode", gx, check)
    y, check = kc.guarded((L, M, B, O), torch.complex64, dev)
    _refused(lib, lib.mk_spec_cmlp_fwd(xd.data_ptr() + 8, wd.data_ptr(), None, y.data_ptr(), *shape, 1, 0, st), "16-byte aligned")
    _untouched("cmlp fwd misaligned x", y, check)
    wr = kc.poisoned(torch.randn(O, I, generator=_gen(12)), dev)
    _refused(lib, lib.mk_spec_mix_fwd(xd.data_ptr(), wr.data_ptr() + 8, y.data_ptr(), *shape, st), "16-byte aligned")
    _untouched("mix fwd misaligned w", y, check)
    _refused(lib, lib.mk_spec_bdmlp_fwd(xd.data_ptr(), wd.data_ptr(), y.data_ptr() + 8, L * M * B, 1, I, O, 0, 0.0, st), "16-byte aligned")
    _untouched("bdmlp fwd misaligned y", y, check)
    xf = kc.poisoned(_crand(_gen(13), 8, 4), dev)
    tab = _dft_table(lib, dev, 8, 8)
    out, check = kc.guarded((8, 4), torch.complex64, dev)
    _refused(lib, lib.mk_latdft_fwd(xf.data_ptr(), tab.data_ptr() + 4, out.data_ptr(), 8, 8, 4, st), "16-byte aligned")
    _untouched("latdft misaligned table", out, check)


# ---------------------------------------------------------------------------------------------------------------------
# the real channel mix (a tile is 64 complex rows)
# ---------------------------------------------------------------------------------------------------------------------
MIX = [
    (66, 67, 1, 6, 34, 0, 0),
    (4, 35, 2, 34, 130, 40, 0),      # 70 rows; I = 34: even, no multiple of 4 (Row2Stager's 8-byte path); two column tiles; dgrad: TransStager
    (384, 3, 1, 130, 130, 0, 2),     # wgrad: two degrees per workgroup, the first group has no rows at all
]


@pytest.mark.parametrize("shape", MIX, ids=["x".join(map(str, s)) for s in MIX])
def test_spec_mix(dev, shape):
    """Forward, data gradient and the atomic weight gradient.  The weight gradient is zeroed inside its guarded view; at most
    one workgroup per degree adds to an element, so the slack is that of a sum of (degrees with rows) terms."""
    from makani_amd import _lib, ops
    lib = _lib.load()
    L, M, B, I, O, l_off, m_off = shape
    g = _gen(14, *shape)
    x64, xd, valid = _spectrum(g, dev, L, M, B, I, l_off, m_off)
    gy64, gyd, _ = _spectrum(g, dev, L, M, B, O, l_off, m_off)
    w = torch.randn(O, I, generator=g)
    wd, w64, st = kc.poisoned(w, dev), w.double(), ops._stream()
    wc = w64.to(torch.complex128)
    y, check = kc.guarded((L, M, B, O), torch.complex64, dev)
    _lib.check(lib.mk_spec_mix_fwd(xd.data_ptr(), wd.data_ptr(), y.data_ptr(), *shape, st), "mk_spec_mix_fwd")
    _check(f"mix fwd {shape}", y, check, torch.einsum("lmbi,oi->lmbo", x64, wc), kc.absdot("lmbi,oi->lmbo", x64, w64), valid)
    gx, check = kc.guarded((L, M, B, I), torch.complex64, dev)
    _lib.check(lib.mk_spec_mix_dgrad(gyd.data_ptr(), wd.data_ptr(), gx.data_ptr(), *shape, st), "mk_spec_mix_dgrad")
    _check(f"mix dgrad {shape}", gx, check, torch.einsum("lmbo,oi->lmbi", gy64, wc), kc.absdot("lmbo,oi->lmbi", gy64, w64), valid)
    gw, check = kc.guarded((O, I), torch.float32, dev)
    gw.zero_()
    _lib.check(lib.mk_spec_mix_wgrad(xd.data_ptr(), gyd.data_ptr(), gw.data_ptr(), *shape, st), "mk_spec_mix_wgrad")
    ref = torch.einsum("lmbo,lmbi->oi", gy64, x64.conj()).real
    mag = kc.absdot("lmbo,lmbi->oi", gy64, x64).real
    degrees = int(valid.flatten(1).any(1).sum())
    torch.cuda.synchronize()
    check(f"mix wgrad {shape}")
    slack = kc.x3_slack_sum(degrees, mag)
    worst = kc.x3_elementwise(gw.cpu(), ref, mag, slack64=slack, what=f"mix wgrad {shape}")
    print(f"[x3 guard] mix wgrad {shape} ({degrees} degrees with rows): worst ratio {worst:.2f} of {kc.X3_C}{_raw_ratio(gw.cpu(), ref, mag, slack)}, "
          f"worst row {_worst_row(gw.cpu(), ref, torch.ones(O, I, dtype=torch.bool)):.2e}")


# ---------------------------------------------------------------------------------------------------------------------
# the block-diagonal MLP on the dense spectrum
# ---------------------------------------------------------------------------------------------------------------------
BD = [(1, 1, 2, 2), (129, 3, 6, 34), (70, 2, 130, 66), (4100, 2, 6, 34)]       # (rows, nb, ib, ob)
LAMBDA = 0.5


def _shrink(v, lam):
    return torch.where(v > lam, v - lam, torch.where(v < -lam, v + lam, torch.zeros((), dtype=v.dtype)))


@pytest.mark.parametrize("rows,nb,ib,ob", BD)
def test_bdmlp(dev, rows, nb, ib, ob):
    from makani_amd import _lib, ops
    lib = _lib.load()
    case, st = (rows, nb, ib, ob), ops._stream()
    g = _gen(15, *case)
    x, gy, a, w = _crand(g, rows, nb, ib), _crand(g, rows, nb, ob), _crand(g, rows, nb, ib), _crand(g, nb, ib, ob)
    xd, gyd, ad, wd = (kc.poisoned(t, dev) for t in (x, gy, a, w))
    x64, gy64, a64, w64 = (_c128(t) for t in (x, gy, a, w))
    pre, mag = torch.einsum("rki,kio->rko", x64, w64), kc.absdot("rki,kio->rko", x64, w64)
    lam32 = float(torch.tensor(LAMBDA, dtype=torch.float32))
    for act in (0, 2, 3):
        ref = {0: pre, 2: _relu_parts(pre, True, True), 3: torch.complex(_shrink(pre.real, lam32), _shrink(pre.imag, lam32))}[act]
        y, check = kc.guarded((rows, nb, ob), torch.complex64, dev)
        _lib.check(lib.mk_spec_bdmlp_fwd(xd.data_ptr(), wd.data_ptr(), y.data_ptr(), *case, act, LAMBDA, st), "mk_spec_bdmlp_fwd")
        _check(f"bdmlp fwd {case} act={act}", y, check, ref, mag, slack=kc.x3_slack_add(ref) if act == 3 else None)
    full, mag = torch.einsum("rko,kio->rki", gy64, w64.conj()), kc.absdot("rko,kio->rki", gy64, w64)
    zero = torch.zeros((), dtype=torch.float64)
    for act in (0, 2):
        ref = full if act == 0 else torch.complex(torch.where(a64.real > 0, full.real, zero), torch.where(a64.imag > 0, full.imag, zero))
        gx, check = kc.guarded((rows, nb, ib), torch.complex64, dev)
        _lib.check(lib.mk_spec_bdmlp_dgrad(gyd.data_ptr(), wd.data_ptr(), ad.data_ptr() if act else None, gx.data_ptr(), *case, act, st),
                   "mk_spec_bdmlp_dgrad")
        _check(f"bdmlp dgrad {case} act={act}", gx, check, ref, mag)
    # weight gradient: row groups into partial panels, added in a fixed order
    nbytes = lib.mk_spec_bdmlp_wgrad_workspace(*case)
    panel = nb * ib * ob * 8
    assert nbytes % panel == 0
    if rows == 4100:
        assert nbytes == 129 * panel, "4100 rows are 129 groups of 32 rows, the last with 4"
    groups = max(nbytes // panel, 1)
    ref, mag = torch.einsum("rki,rko->kio", x64.conj(), gy64), kc.absdot("rki,rko->kio", x64, gy64)
    runs = []
    for _ in range(2):
        ws, wsp = _workspace(nbytes, dev)
        gw, check = kc.guarded((nb, ib, ob), torch.complex64, dev)
        _lib.check(lib.mk_spec_bdmlp_wgrad(xd.data_ptr(), gyd.data_ptr(), gw.data_ptr(), wsp, *case, st), "mk_spec_bdmlp_wgrad")
        runs.append(_check(f"bdmlp wgrad {case} ({groups} panels)", gw, check, ref, mag,
                           slack=kc.x3_slack_sum(groups, mag) if groups > 1 else None))
    assert torch.equal(torch.view_as_real(runs[0]), torch.view_as_real(runs[1])), "the block weight gradient differs between two runs"
    # the soft-shrink mask, out aliasing gy: exact
    s = torch.complex(_shrink(pre.real, lam32), _shrink(pre.imag, lam32)).to(torch.complex64)
    sd = kc.poisoned(s, dev)
    out, check = kc.guarded((rows, nb, ob), torch.complex64, dev)
    out.copy_(gy)
    _lib.check(lib.mk_spec_bdmlp_mask(out.data_ptr(), sd.data_ptr(), out.data_ptr(), rows * nb * ob * 2, st), "mk_spec_bdmlp_mask")
    torch.cuda.synchronize()
    check(f"bdmlp mask {case}")
    want = torch.where(torch.view_as_real(s) != 0, torch.view_as_real(gy), torch.zeros(()))
    assert torch.equal(torch.view_as_real(out.cpu()), want), f"bdmlp mask {case}"
