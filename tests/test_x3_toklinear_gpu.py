"""The fp32 token-major linear family on the bf16x3 engine (csrc/x3_toklinear.hip) through the C ABI, held to the checks of
tests/test_x3_guard_gpu.py (helpers in tests/kernel_checks.py):

* every written element passes ``x3_elementwise`` against a float64 einsum of the same inputs, with ``x3_slack_add`` per extra
  epilogue addition and ``x3_slack_sum`` for the weight gradient's panels; the constant is ``X3_C``, from the CPU emulation;
* GELU-bearing outputs: ``gelu`` and ``gelu'`` are bounded by ``GELU_GRAD_MAX``, so the bound of the argument is scaled by it,
  and the activation's own fp32 rounding is added with the constants of tests/test_x3_toklinear_cpu.py (``GELU_ROUND_C``,
  ``GELU_GRAD_ROUND_C``: the fp32 expression in torch against float64, doubled -- never the kernel's).  These rows are also
  held to 1e-5 per row (``row_rel``), as tests/test_conv_guard_gpu.py holds its GELU rows;
* every output lies between sentinel bands, every row stride is wider than the row and the gap columns keep the sentinel;
* x, w, bias, addend and aux lie between NaN bands and have NaN gap columns: a read past a row's end shows up as a NaN.

Contraction lengths stay at or below 280, where a single dropped piece product still lies three times over ``X3_C``."""
import pytest
import torch

import kernel_checks as kc
from test_x3_toklinear_cpu import GELU_GRAD_ROUND_C, GELU_ROUND_C, WGRAD_SHAPES, FWD_SHAPES

pytestmark = pytest.mark.gpu

GAP = 4
ROW_TOL = 1e-5
U = 2.0 ** -23


def _strided_nan(t, dev):
    """``t`` [rows, n] as rows of length n + GAP whose gap columns are NaN, between NaN bands."""
    full = torch.full((t.shape[0], t.shape[1] + GAP), float("nan"), dtype=t.dtype)
    full[:, :t.shape[1]] = t
    return kc.poisoned(full, dev)


def _out(rows, n, dev):
    return kc.guarded((rows, n + GAP), torch.float32, dev)


def _check(name, out, check, n, ref, mag, slack=None, row_tol=None):
    """Bands intact, gap columns still the sentinel, no written element the sentinel, every element inside the criterion."""
    torch.cuda.synchronize()
    check(name)
    y = out.detach().cpu()
    assert bool((y[:, n:].contiguous().view(torch.int32) == torch.tensor([kc.SENTINEL]).view(torch.int32)).all()), f"{name}: a gap column was written"
    got = y[:, :n]
    assert not bool((got == kc.SENTINEL).any()), f"{name}: an element the contract writes still holds the sentinel"
    worst = kc.x3_elementwise(got, ref, mag, slack64=slack, what=name)
    rr = float(kc.row_rel(got.double().numpy(), ref.numpy()).max())
    print(f"[x3 toklinear] {name}: worst ratio {worst:.2f} of {kc.X3_C}, worst row {rr:.2e}")
    if row_tol is not None:
        assert rr < row_tol, f"{name}: worst row {rr:.2e}"
    return got


def _p(t):
    return None if t is None else t.data_ptr()


def _fwd(lib, x, ldx, w, ldw, kmajor, bias, y, pre, addend, aux, act, R, O, I, ld_o):
    from makani_amd import ops
    return lib.mk_token_linear_x3_fwd(_p(x), ldx, _p(w), ldw, kmajor, _p(bias), _p(y), ld_o, _p(pre), ld_o if pre is not None else 0,
                                      _p(addend), ld_o if addend is not None else 0, _p(aux), ld_o if aux is not None else 0, act,
                                      R, O, I, ops._stream())


class _Case:
    """Inputs of one (R, I, O, kmajor) on the device and their float64 references (computed once per case)."""

    def __init__(self, dev, R, I, O, kmajor):
        g = torch.Generator().manual_seed(1000 * R + 10 * I + O + kmajor)
        self.R, self.I, self.O, self.kmajor = R, I, O, kmajor
        x = torch.randn(R, I, generator=g)
        w = torch.randn(O, I, generator=g) / I ** 0.5           # logically [O, I]; stored [I, O] for kmajor
        bias, addend, aux = torch.randn(O, generator=g), torch.randn(R, O, generator=g), 1.5 * torch.randn(R, O, generator=g)
        self.x, self.ldx = _strided_nan(x, dev), I + GAP
        self.w, self.ldw = (_strided_nan(w.t().contiguous(), dev), O + GAP) if kmajor else (_strided_nan(w, dev), I + GAP)
        self.bias, self.addend, self.aux = kc.poisoned(bias, dev), _strided_nan(addend, dev), _strided_nan(aux, dev)
        self.acc = torch.einsum("rk,ok->ro", x.double(), w.double())
        self.mag = kc.absdot("rk,ok->ro", x, w)
        self.b64, self.add64, self.aux64 = bias.double(), addend.double(), aux.double()


@pytest.mark.parametrize("kmajor", [0, 1])
@pytest.mark.parametrize("R,I,O", FWD_SHAPES)
def test_fwd_guarded(dev, R, I, O, kmajor):
    from makani_amd import _lib
    lib = _lib.load()
    c = _Case(dev, R, I, O, kmajor)
    ld_o = O + GAP
    tag = f"fwd {(R, I, O)} kmajor={kmajor}"

    def launch(name, bias=None, pre=False, addend=None, aux=None, act=0):
        y, cy = _out(R, O, dev)
        p, cp = _out(R, O, dev) if pre else (None, None)
        _lib.check(_fwd(lib, c.x, c.ldx, c.w, c.ldw, kmajor, bias, y, p, addend, aux, act, R, O, I, ld_o), "mk_token_linear_x3_fwd")
        return y, cy, p, cp

    # plain, and with the bias: one extra fp32 addition
    y, cy, _, _ = launch("plain")
    _check(f"{tag} plain", y, cy, O, c.acc, c.mag)
    pre64 = c.acc + c.b64
    y, cy, _, _ = launch("bias", bias=c.bias)
    _check(f"{tag} bias", y, cy, O, pre64, c.mag, slack=kc.x3_slack_add(pre64))
    # bias, stored pre-activation and GELU: pre is the bias row's value; gelu is GELU_GRAD_MAX-Lipschitz, so the bound of pre is
    # scaled by it, and the fp32 evaluation of the activation adds GELU_ROUND_C 2^-23 |pre|
    y, cy, p, cp = launch("gelu", bias=c.bias, pre=True, act=1)
    _check(f"{tag} pre", p, cp, O, pre64, c.mag, slack=kc.x3_slack_add(pre64))
    gslack = kc.GELU_GRAD_MAX * kc.x3_slack_add(pre64) + GELU_ROUND_C * U * pre64.abs()
    got = _check(f"{tag} gelu", y, cy, O, kc.gelu64(pre64), kc.GELU_GRAD_MAX * c.mag, slack=gslack, row_tol=ROW_TOL)
    y2, cy2, _, _ = launch("gelu without pre", bias=c.bias, act=1)
    torch.cuda.synchronize()
    cy2("gelu without pre")
    assert torch.equal(y2[:, :O].cpu(), got), f"{tag}: act differs with and without pre"
    # addend: the bias addition and the addend's
    ref = pre64 + c.add64
    y, cy, _, _ = launch("addend", bias=c.bias, addend=c.addend)
    _check(f"{tag} addend", y, cy, O, ref, c.mag, slack=kc.x3_slack_add(pre64) + kc.x3_slack_add(ref))
    # aux: acc * gelu'(aux): the accumulation's bound times max |gelu'|, the fp32 evaluation of gelu' (absolute
    # GELU_GRAD_ROUND_C 2^-23) times |acc|, and the product's rounding
    ref = c.acc * kc.gelu_grad64(c.aux64)
    y, cy, _, _ = launch("aux", aux=c.aux)
    _check(f"{tag} aux", y, cy, O, ref, kc.GELU_GRAD_MAX * c.mag, slack=GELU_GRAD_ROUND_C * U * c.acc.abs() + kc.x3_slack_add(ref),
           row_tol=ROW_TOL)


def _wgrad_inputs(dev, R, O, I):
    g = torch.Generator().manual_seed(7 * R + O + I)
    dy, x = torch.randn(R, O, generator=g), torch.randn(R, I, generator=g)
    return dy, x, _strided_nan(dy, dev), _strided_nan(x, dev)


@pytest.mark.parametrize("R,O,I", WGRAD_SHAPES)
def test_wgrad_guarded(dev, R, O, I):
    from makani_amd import _lib, ops
    lib = _lib.load()
    dy, x, dyd, xd = _wgrad_inputs(dev, R, O, I)
    ref = torch.einsum("ro,ri->oi", dy.double(), x.double())
    mag = kc.absdot("ro,ri->oi", dy, x)
    db64 = dy.double().sum(0)
    for slabs in (1, 2, 3, 0):
        nbytes = lib.mk_token_linear_x3_wgrad_workspace(R, O, I, slabs)
        assert nbytes > 0 and nbytes % 8 == 0
        used = (nbytes - (R + 127) // 128 * O * 8) // (O * I * 4)          # panels: 0 for one slab
        if slabs:
            assert max(used, 1) == slabs, (slabs, used)
        results = []
        for run in range(2):
            ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=dev)      # every float and double of it reads as NaN
            dw, cw = _out(O, I, dev)
            db, cb = kc.guarded((O,), torch.float32, dev)
            _lib.check(lib.mk_token_linear_x3_wgrad(dyd.data_ptr(), O + GAP, xd.data_ptr(), I + GAP, dw.data_ptr(), I + GAP, db.data_ptr(),
                                                    ws.data_ptr(), R, O, I, slabs, ops._stream()), "mk_token_linear_x3_wgrad")
            name = f"wgrad {(R, O, I)} slabs={slabs} ({max(used, 1)} used)"
            got = _check(name, dw, cw, I, ref, mag, slack=kc.x3_slack_sum(max(used, 1), mag))
            cb(name + " db")
            dbc = db.cpu().double()
            assert bool(torch.isfinite(dbc).all())
            # float64 sums rounded once to fp32
            assert bool(((dbc - db64).abs() <= U * db64.abs() + 2.0 ** -40 * dy.double().abs().sum(0)).all()), f"{name}: db"
            results.append((got.clone(), db.cpu().clone()))
        assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]), f"{name}: two runs differ"
    # without db and with one slab no workspace is needed
    dw, cw = _out(O, I, dev)
    _lib.check(lib.mk_token_linear_x3_wgrad(dyd.data_ptr(), O + GAP, xd.data_ptr(), I + GAP, dw.data_ptr(), I + GAP, None, None, R, O, I, 1,
                                            ops._stream()), "mk_token_linear_x3_wgrad")
    _check(f"wgrad {(R, O, I)} one slab, no db", dw, cw, I, ref, mag)


def test_refusals(dev):
    from makani_amd import _lib, ops
    lib = _lib.load()
    R, I, O = 33, 36, 68
    c = _Case(dev, R, I, O, 0)
    ld_o = O + GAP

    def refused(text, **kw):
        y, cy = _out(R, O, dev)
        p, cp = _out(R, O, dev)
        a = dict(x=c.x.data_ptr(), ldx=c.ldx, w=c.w.data_ptr(), ldw=c.ldw, y=y.data_ptr(), pre=None, act=0, O=O, I=I)
        a.update(kw)
        if a["pre"] == "given":
            a["pre"] = p.data_ptr()
        rc = lib.mk_token_linear_x3_fwd(a["x"], a["ldx"], a["w"], a["ldw"], 0, c.bias.data_ptr(), a["y"], ld_o, a["pre"],
                                        ld_o if a["pre"] else 0, None, 0, None, 0, a["act"], R, a["O"], a["I"], ops._stream())
        msg = lib.mk_last_error().decode()
        assert rc != 0 and text in msg, (rc, msg)
        torch.cuda.synchronize()
        for buf, chk in ((y, cy), (p, cp)):
            chk(text)
            assert bool((buf == kc.SENTINEL).all()), f"{text}: a refused call wrote its output"

    refused("not 16-byte aligned", x=c.x.data_ptr() + 4)
    refused("row stride smaller", ldx=I - 4)
    refused("multiples of 4", I=I + 2)
    refused("multiples of 4", O=O + 2)
    refused("act must be", act=2)
    refused("null pointer", y=None, pre="given", act=1)
    refused("pre is stored only", pre="given")
    # the weight gradient: the same operand checks, before any launch
    dy, x, dyd, xd = _wgrad_inputs(dev, R, O, I)
    dw, cw = _out(O, I, dev)
    ws = torch.empty(lib.mk_token_linear_x3_wgrad_workspace(R, O, I, 2), dtype=torch.uint8, device=dev)
    for text, kw in (("not 16-byte aligned", dict(dy=dyd.data_ptr() + 4)), ("row stride smaller", dict(ldx=I - 4)),
                     ("multiples of 4", dict(I=I + 2)), ("slabs must be", dict(slabs=65)), ("workspace null", dict(ws=None))):
        a = dict(dy=dyd.data_ptr(), ldx=I + GAP, I=I, slabs=2, ws=ws.data_ptr())
        a.update(kw)
        rc = lib.mk_token_linear_x3_wgrad(a["dy"], O + GAP, xd.data_ptr(), a["ldx"], dw.data_ptr(), I + GAP, None, a["ws"], R, O, a["I"],
                                          a["slabs"], ops._stream())
        msg = lib.mk_last_error().decode()
        assert rc != 0 and text in msg, (rc, msg)
        torch.cuda.synchronize()
        cw(text)
        assert bool((dw == kc.SENTINEL).all()), f"{text}: a refused call wrote dw"
    assert lib.mk_token_linear_x3_wgrad_workspace(R, O, I + 2, 0) == -1


def test_capture_replay_bit_equal(dev):
    """Forward, data gradient and weight gradient at (33, 36, 68) captured into one graph: the replay gives the eager bits."""
    from makani_amd import _lib, ops
    lib = _lib.load()
    R, I, O = 33, 36, 68
    g = torch.Generator().manual_seed(3)
    x, w, b, gy = (torch.randn(*s, generator=g).to(dev) for s in ((R, I), (O, I), (O,), (R, O)))
    nbytes = lib.mk_token_linear_x3_wgrad_workspace(R, O, I, 2)

    def step(y, dx, dw, db, ws):
        st = ops._stream()
        _lib.check(lib.mk_token_linear_x3_fwd(x.data_ptr(), I, w.data_ptr(), I, 0, b.data_ptr(), y.data_ptr(), O, None, 0, None, 0, None, 0, 0,
                                              R, O, I, st), "fwd")
        _lib.check(lib.mk_token_linear_x3_fwd(gy.data_ptr(), O, w.data_ptr(), I, 1, None, dx.data_ptr(), I, None, 0, None, 0, None, 0, 0,
                                              R, I, O, st), "dgrad")
        _lib.check(lib.mk_token_linear_x3_wgrad(gy.data_ptr(), O, x.data_ptr(), I, dw.data_ptr(), I, db.data_ptr(), ws.data_ptr(), R, O, I, 2,
                                                st), "wgrad")

    def buffers():
        return (torch.zeros(R, O, device=dev), torch.zeros(R, I, device=dev), torch.zeros(O, I, device=dev), torch.zeros(O, device=dev),
                torch.zeros(nbytes, dtype=torch.uint8, device=dev))

    eager = buffers()
    step(*eager)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    static = buffers()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*static)                                     # warm-up on the capture stream
    side.synchronize()
    for t in static:
        t.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step(*static)
    graph.replay()
    torch.cuda.synchronize()
    for name, a, e in zip(("y", "dx", "dw", "db"), static, eager):
        assert torch.equal(a, e), f"{name}: the replay differs from the eager run"
    assert float(eager[0].abs().sum()) > 0 and float(eager[2].abs().sum()) > 0
