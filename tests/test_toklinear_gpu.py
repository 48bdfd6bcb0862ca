"""The token-major linear kernels (csrc/toklinear.hip) through the C ABI with the criteria of tests/kernel_checks.py and the
bounds of tests/toklinear_checks.py: every element against a float64 reference on the same bf16-rounded operands, outputs
between sentinel bands with the sentinel kept in an 8-element gap behind every row, inputs between NaN bands with NaN in their
gaps, every launch run a second time and compared bit for bit, error returns that launch nothing.

Shapes come from mk_token_linear_info.  Not the full product: one axis varies around its tile while the others sit at a ragged
value, plus one case ragged and longer in all three axes."""
import pytest
import torch

import kernel_checks as kc
import toklinear_checks as tc

pytestmark = pytest.mark.gpu

GAP = 8
BF, F32 = torch.bfloat16, torch.float32


def _info():
    from makani_amd import ops
    return ops.token_linear_info()


def _fwd_cases():
    t = _info()
    tr, tcol, tk = t["tr"], t["tc"], t["tk"]
    R0, O0, I0 = tr + 1, tcol + 8, tk + 8
    cases = [(R, O0, I0) for R in (1, tr - 1, tr, tr + 1, 2 * tr + 3)]
    cases += [(R0, O, I0) for O in (8, tcol - 8, tcol, tcol + 8)]
    cases += [(R0, O0, I) for I in (8, tk - 8, tk, tk + 8, 2 * tk + 8)]
    cases += [(2 * tr + 3, tcol + 8, 2 * tk + 8)]
    return sorted(set(cases))


def _wgrad_cases():
    t = _info()
    to, ti, ts = t["to"], t["ti"], t["ts"]
    O0, I0 = to + 8, ti - 8
    cases = [(R, O0, I0, s) for R in (1, ts - 1, ts + 1, 2 * ts + 3, 5 * ts + 1) for s in (1, 2, 3)]
    cases += [(2 * ts + 3, O, I0, 2) for O in (8, to - 8, to, to + 8)]
    cases += [(2 * ts + 3, O0, I, 2) for I in (8, ti - 8, ti, ti + 8)]
    cases += [(5 * ts + 1, O0, I0, 0), (40 * ts + 5, 16, 24, 0)]          # slabs chosen by the library
    return sorted(set(cases))


def _rand(gen, *shape, scale=1.0, shift=0.0, dtype=BF):
    return (torch.randn(*shape, generator=gen, dtype=torch.float64) * scale + shift).to(dtype)


def _gapped_in(t, dev):
    """``t`` ``[rows, L]`` on the device with NaN in an 8-element gap behind every row and NaN bands around: (view, ld)."""
    host = torch.full((t.shape[0], t.shape[1] + GAP), float("nan"), dtype=t.dtype)
    host[:, :t.shape[1]] = t
    return kc.poisoned(host, dev), t.shape[1] + GAP


class Out:
    """A guarded ``[rows, L]`` output with the 8-element gap: the sentinel must survive in the gap and in the bands."""

    def __init__(self, rows, L, dtype, dev):
        self.L, self.ld = L, L + GAP
        self.buf, self.bands = kc.guarded((rows, L + GAP), dtype, dev)

    def ptr(self):
        return self.buf.data_ptr()

    def take(self, what):
        """The result on the host, after the checks of the gap and the bands."""
        self.bands(what)
        host = self.buf.cpu()
        assert bool((host[:, self.L:] == kc.SENTINEL).all()), f"{what}: the gap behind a row was written"
        return host[:, :self.L].clone()

    def untouched(self, what):
        self.bands(what)
        assert bool((self.buf.cpu() == kc.SENTINEL).all()), f"{what}: a refused call wrote its output"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from makani_amd import _lib as L
    return L.load()


def _p(t):
    return None if t is None else (t.ptr() if isinstance(t, Out) else t.data_ptr())


def _fwd(x, ldx, w, ldw, bias, R, O, I, y=None, act=None, pre=None, addend=None, ldadd=0, out=None, aux=None, ldaux=0):
    def ld(o):
        return 0 if o is None else o.ld
    return _lib().mk_token_linear_fwd(x.data_ptr(), ldx, w.data_ptr(), ldw, _p(bias), _p(y), ld(y), _p(act), ld(act), _p(pre), ld(pre),
                                      _p(addend), ldadd, _p(out), ld(out), _p(aux), ldaux, R, O, I, _stream())


def _twice(launch, outs, what):
    """Run ``launch`` into fresh outputs twice; returns the first results after comparing the second bit for bit."""
    first = None
    for run in range(2):
        bufs = outs()
        assert launch(*bufs) == 0, f"{what}: {_lib().mk_last_error().decode()}"
        got = [b.take(f"{what} run {run}") for b in bufs]
        if first is None:
            first = got
        else:
            for a, b in zip(first, got):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{what}: two runs differ"
    return first


@pytest.mark.parametrize("R,O,I", _fwd_cases())
def test_forward_every_epilogue(dev, R, O, I):
    gen = torch.Generator().manual_seed(1000 * R + 10 * O + I)
    x, w = _rand(gen, R, I), _rand(gen, O, I, scale=I ** -0.5)
    b = _rand(gen, O, scale=0.5, dtype=F32)
    addend, aux = _rand(gen, R, O, dtype=F32), _rand(gen, R, O)
    xd, ldx = _gapped_in(x, dev)
    wd, ldw = _gapped_in(w, dev)
    bd = kc.poisoned(b, dev)
    ad, ldadd = _gapped_in(addend, dev)
    auxd, ldaux = _gapped_in(aux, dev)
    ref, ref0 = tc.Ref(x, w, b), tc.Ref(x, w)
    what = f"R={R} O={O} I={I}"

    def bf():
        return Out(R, O, BF, dev)

    (y,) = _twice(lambda o: _fwd(xd, ldx, wd, ldw, bd, R, O, I, y=o), lambda: [bf()], what + " plain")
    print(what, "plain", tc.check_plain(y, ref, what + " plain"))
    (y0,) = _twice(lambda o: _fwd(xd, ldx, wd, ldw, None, R, O, I, y=o), lambda: [bf()], what + " no bias")
    print(what, "no bias", tc.check_plain(y0, ref0, what + " no bias"))

    act, pre = _twice(lambda a, p: _fwd(xd, ldx, wd, ldw, bd, R, O, I, act=a, pre=p), lambda: [bf(), bf()], what + " gelu")
    print(what, "pre", tc.check_pre(pre, ref, what + " pre"))
    print(what, "act", tc.check_act(act, pre, what + " act"))
    (act1,) = _twice(lambda a: _fwd(xd, ldx, wd, ldw, bd, R, O, I, act=a), lambda: [bf()], what + " gelu without pre")
    assert torch.equal(act.view(torch.int16), act1.view(torch.int16)), f"{what}: act differs with and without the pre store"

    (out,) = _twice(lambda o: _fwd(xd, ldx, wd, ldw, bd, R, O, I, addend=ad, ldadd=ldadd, out=o), lambda: [Out(R, O, F32, dev)],
                    what + " addend")
    print(what, "addend", tc.check_addend(out, addend, ref, what + " addend"))

    (ya,) = _twice(lambda o: _fwd(xd, ldx, wd, ldw, None, R, O, I, y=o, aux=auxd, ldaux=ldaux), lambda: [bf()], what + " aux")
    print(what, "aux", tc.check_aux(ya, ref0, aux, what + " aux"))


@pytest.mark.parametrize("O,I", [(8, 8), (72, 136), (136, 72), (64, 64), (200, 56)])
@pytest.mark.parametrize("dtype", [F32, BF])
def test_pack_rounds_to_nearest_even_both_ways(dev, O, I, dtype):
    gen = torch.Generator().manual_seed(O * 1000 + I)
    w = _rand(gen, O, I, dtype=dtype)
    wd, ldw = _gapped_in(w, dev)
    want = w.to(BF)
    for transpose in (0, 1):
        rows, L = (I, O) if transpose else (O, I)
        (img,) = _twice(lambda o: _lib().mk_token_linear_pack(wd.data_ptr(), 0 if dtype == F32 else 1, ldw, o.ptr(), o.ld, O, I, transpose,
                                                              _stream()), lambda: [Out(rows, L, BF, dev)], f"pack {O}x{I} t={transpose}")
        assert torch.equal(img.view(torch.int16), (want.T if transpose else want).contiguous().view(torch.int16))


@pytest.mark.parametrize("R,O", [(1, 8), (67, 136), (300, 24)])
def test_gelu_grad_pass(dev, R, O):
    """``bf16(g gelu'(pre))``: one bf16 ulp plus the error of the fp32 factor -- 0.75e-7 absolute on the CDF (csrc/gelu.h), the
    rounding of the density and of four fp32 operations, together under ``2^-21 |g| (1 + |pre|)``."""
    gen = torch.Generator().manual_seed(R + O)
    g, pre = _rand(gen, R, O), _rand(gen, R, O, scale=1.5)
    gd, ldg = _gapped_in(g, dev)
    pd, ldp = _gapped_in(pre, dev)
    (out,) = _twice(lambda o: _lib().mk_token_linear_gelu_grad(gd.data_ptr(), ldg, pd.data_ptr(), ldp, o.ptr(), o.ld, R, O, _stream()),
                    lambda: [Out(R, O, BF, dev)], f"gelu grad {R}x{O}")
    g64, p64 = g.double(), pre.double()
    kc.bf16_elementwise(out, g64 * kc.gelu_grad64(p64), 2.0 ** -21 * g64.abs() * (1 + p64.abs()), "gelu grad")


@pytest.mark.parametrize("R,O,I,slabs", _wgrad_cases())
def test_weight_gradient_every_element(dev, R, O, I, slabs):
    gen = torch.Generator().manual_seed(R * 7 + O * 3 + I + slabs)
    dy, x = _rand(gen, R, O, shift=0.5), _rand(gen, R, I)            # a nonzero column mean: db is no sum near zero
    dyd, lddy = _gapped_in(dy, dev)
    xd, ldx = _gapped_in(x, dev)
    lib = _lib()
    nbytes = lib.mk_token_linear_wgrad_workspace(R, O, I, slabs)
    assert nbytes >= 0
    if slabs > 1:
        assert nbytes == slabs * (O * I + O) * 4
    ws = torch.full((nbytes // 4 + 4,), float("nan"), dtype=F32, device=dev)      # the workspace need not be cleared
    what = f"wgrad R={R} O={O} I={I} slabs={slabs}"

    def launch(dw, db):
        return lib.mk_token_linear_wgrad(dyd.data_ptr(), lddy, xd.data_ptr(), ldx, dw.ptr(), dw.ld, db.ptr(), ws.data_ptr(), R, O, I, slabs,
                                         _stream())

    dw, db = _twice(launch, lambda: [Out(O, I, F32, dev), Out(1, O, F32, dev)], what)
    print(what, "dW", tc.check_wgrad(dw, dy, x, what + " dW"), "db", tc.check_dbias(db[0], dy, what + " db"))
    # without db: dW has the same bits
    (dw1,) = _twice(lambda o: lib.mk_token_linear_wgrad(dyd.data_ptr(), lddy, xd.data_ptr(), ldx, o.ptr(), o.ld, None, ws.data_ptr(), R, O, I,
                                                        slabs, _stream()), lambda: [Out(O, I, F32, dev)], what + " no db")
    assert torch.equal(dw.view(torch.int32), dw1.view(torch.int32))


def test_row_offsets_past_2_to_31_elements(dev):
    """20 000 rows at a stride of 2^17 elements: rows from 16 384 on start 2^31 elements or more behind the first (18 % of the
    tokens, so that the weight gradient's bound, which grows with R, still sees them missing or misread).  The forward kernel is
    checked on the first and the last rows, the weight gradient as a whole."""
    R, LD, I, O = 20000, 2 ** 17, 16, 8
    gen = torch.Generator().manual_seed(77)
    x, w, dy = _rand(gen, R, I), _rand(gen, O, I, scale=0.25), _rand(gen, R, O, shift=0.5)
    xd = torch.full((R * LD,), float("nan"), dtype=BF, device=dev).view(R, LD)
    xd[:, :I] = x.to(dev)
    yd = torch.full((R * LD,), kc.SENTINEL, dtype=BF, device=dev).view(R, LD)
    wd = w.to(dev).contiguous()
    lib = _lib()
    assert lib.mk_token_linear_fwd(xd.data_ptr(), LD, wd.data_ptr(), I, None, yd.data_ptr(), LD, None, 0, None, 0, None, 0, None, 0, None, 0,
                                   R, O, I, _stream()) == 0
    for rows in (slice(0, 300), slice(R - 300, R)):
        got = yd[rows, :O + GAP].cpu()
        assert bool((got[:, O:] == kc.SENTINEL).all())
        tc.check_plain(got[:, :O], tc.Ref(x[rows], w), f"rows {rows}")
    # the weight gradient of the same rows: dY rides in the output buffer's rows
    yd[:, :O] = dy.to(dev)
    dw, db = Out(O, I, F32, dev), Out(1, O, F32, dev)
    nbytes = lib.mk_token_linear_wgrad_workspace(R, O, I, 3)
    ws = torch.empty(nbytes // 4, dtype=F32, device=dev)
    assert lib.mk_token_linear_wgrad(yd.data_ptr(), LD, xd.data_ptr(), LD, dw.ptr(), dw.ld, db.ptr(), ws.data_ptr(), R, O, I, 3, _stream()) == 0
    tc.check_wgrad(dw.take("dW"), dy, x, "dW at 2^31")
    tc.check_dbias(db.take("db")[0], dy, "db at 2^31")
    del xd, yd
    torch.cuda.empty_cache()


def test_refusals_launch_nothing(dev):
    R, O, I = 40, 24, 16
    gen = torch.Generator().manual_seed(5)
    x, w = _rand(gen, R, I + 8), _rand(gen, O, I + 8)
    xd, wd = kc.poisoned(x, dev), kc.poisoned(w, dev)
    b = kc.poisoned(_rand(gen, O, dtype=F32), dev)
    add = kc.poisoned(_rand(gen, R, O, dtype=F32), dev)
    lib = _lib()

    def refused(what, **kw):
        args = dict(x=xd.data_ptr(), ldx=I + 8, w=wd.data_ptr(), ldw=I + 8, bias=None, R=R, O=O, I=I, mode="y")
        args.update(kw)
        y, act, outf = Out(R, O, BF, dev), Out(R, O, BF, dev), Out(R, O, F32, dev)
        m = args["mode"]
        rc = lib.mk_token_linear_fwd(args["x"], args["ldx"], args["w"], args["ldw"], _p(args["bias"]),
                                     y.ptr() if "y" in m else None, y.ld, act.ptr() if "a" in m else None, act.ld,
                                     act.ptr() if "p" in m else None, act.ld, add.data_ptr() if "d" in m else None, O,
                                     outf.ptr() if "f" in m else None, outf.ld, xd.data_ptr() if "x" in m else None, I + 8,
                                     args["R"], args["O"], args["I"], _stream())
        assert rc == 1, f"{what}: code {rc}"
        assert lib.mk_last_error()
        for o in (y, act, outf):
            o.untouched(what)

    refused("I % 8", I=12)
    refused("O % 8", O=20)
    refused("ld < row length", ldx=I - 8)
    refused("ld % 8", ldw=I + 4)
    refused("misaligned x", x=xd.data_ptr() + 2)
    refused("misaligned bias", bias=b[1:])
    refused("R = 0", R=0)
    refused("y and act", mode="ya")
    refused("pre without act", mode="yp")
    refused("addend without out", mode="d")
    refused("addend with y", mode="ydf")
    refused("aux with bias", mode="yx", bias=b)
    refused("aux with act", mode="ax")
    refused("nothing", mode="")

    dw = Out(O, I, F32, dev)
    ws = torch.empty(4 * (O * I + O), dtype=F32, device=dev)
    for what, kw in (("wgrad I % 8", dict(I=12)), ("wgrad ld", dict(ldx=8)), ("wgrad slabs", dict(slabs=65)),
                     ("wgrad misaligned", dict(x=xd.data_ptr() + 2)), ("wgrad no workspace", dict(ws=None))):
        a = dict(x=xd.data_ptr(), ldx=I + 8, I=I, slabs=2, ws=ws.data_ptr())
        a.update(kw)
        rc = lib.mk_token_linear_wgrad(add.data_ptr(), O, a["x"], a["ldx"], dw.ptr(), dw.ld, None, a["ws"], R, O, a["I"], a["slabs"], _stream())
        assert rc == 1, f"{what}: code {rc}"
        dw.untouched(what)
    assert lib.mk_token_linear_wgrad_workspace(R, O, 12, 1) == -1

    img = Out(O, I, BF, dev)
    for what, kw in (("pack dtype", dict(dtype=2)), ("pack ld", dict(ldo=I - 8)), ("pack I % 8", dict(I=12))):
        a = dict(dtype=1, ldo=img.ld, I=I)
        a.update(kw)
        assert lib.mk_token_linear_pack(wd.data_ptr(), a["dtype"], I + 8, img.ptr(), a["ldo"], O, a["I"], 0, _stream()) == 1, what
        img.untouched(what)


def test_info_needs_no_launch():
    t = _info()
    assert set(t) == {"tr", "tc", "tk", "to", "ti", "ts"} and all(v > 0 and v % 8 == 0 for v in t.values())
