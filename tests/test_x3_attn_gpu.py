"""The fp32 attention kernels (csrc/x3_attn.hip) through the C ABI with the criteria of tests/kernel_checks.py and the bounds of
tests/x3_attn_checks.py: every element of o, lse, dq, dk, dv against the float64 reference, outputs (delta too) between sentinel
bands (and, in the packed layout, with the sentinel kept in a gap between rows), inputs between NaN bands (and NaN in their
gaps), a second run compared bit for bit, error returns that launch nothing.

Token counts come from mk_attn_x3_info: for each (query tile tq, key tile tk) of the three kernels
{1, tk - 1, tk, tk + 1, tq + 1, 2 max(tq, tk) + 3} with Nq = Nk, plus Nq = tq + 1, Nk = 2 tk + 3 and the two swapped.
B = 2, H = 3: batch and head strides are both exercised.  Head sizes: those of {16, 48, 64, 128} the kernels support."""
import ctypes
import math

import pytest
import torch

import attn_checks as ac
import kernel_checks as kc
import x3_attn_checks as xc

pytestmark = pytest.mark.gpu

B, H, GAP = 2, 3, 8
F32 = torch.float32


def _tiles(D):
    from makani_amd import ops
    return ops.attn_x3_info(D)


def _heads():
    from makani_amd import ops
    return [D for D in (16, 48, 64, 128) if D <= ops.ATTN_X3_MAX_HEAD]


def _counts(D):
    n = set()
    for tq, tk in _tiles(D):
        n |= {1, tk - 1, tk, tk + 1, tq + 1, 2 * max(tq, tk) + 3}
    return sorted(n)


def _cases():
    """(D, Nq, Nk, layout): sized from the tile sizes, which the library reports without a device."""
    out = []
    for D in _heads():
        for n in _counts(D):
            out += [(D, n, n, "packed"), (D, n, n, "bhnd")]
        (tq, tk) = _tiles(D)[0]
        out += [(D, tq + 1, 2 * tk + 3, "bhnd"), (D, 2 * tk + 3, tq + 1, "bhnd")]
    return out


def _arr(vals):
    return (ctypes.c_longlong * len(vals))(*vals)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


class Problem:
    """One set of fp32 operands on the device in one layout; every launch writes into fresh guarded buffers."""

    def __init__(self, dev, q, k, v, go, layout):
        from makani_amd import _lib
        self.lib, self.dev, self.layout = _lib.load(), dev, layout
        self.Nq, self.Nk, self.D = q.shape[2], k.shape[2], q.shape[3]
        D, Nq, Nk = self.D, self.Nq, self.Nk
        self.scale = 1.0 / math.sqrt(D)
        nan = float("nan")
        if layout == "bhnd":
            self.q, self.k, self.v, self.go = (kc.poisoned(t, dev) for t in (q, k, v, go))
            self.in_ptr = [t.data_ptr() for t in (self.q, self.k, self.v)]
            self.in_str = [(H * Nq * D, Nq * D, D), (H * Nk * D, Nk * D, D), (H * Nk * D, Nk * D, D)]
            self.go_ptr, self.go_str = self.go.data_ptr(), (H * Nq * D, Nq * D, D)
        else:
            assert Nq == Nk
            self.W, self.Wo = 3 * H * D + GAP, H * D + GAP
            x = torch.full((B, Nq, self.W), nan, dtype=F32)
            x[..., :3 * H * D] = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B, Nq, 3 * H * D)
            g = torch.full((B, Nq, self.Wo), nan, dtype=F32)
            g[..., :H * D] = go.permute(0, 2, 1, 3).reshape(B, Nq, H * D)
            self.qkv, self.go = kc.poisoned(x, dev), kc.poisoned(g, dev)
            self.in_ptr = [self.qkv.data_ptr() + 4 * i * H * D for i in range(3)]
            self.in_str = [(Nq * self.W, D, self.W)] * 3
            self.go_ptr, self.go_str = self.go.data_ptr(), (Nq * self.Wo, D, self.Wo)

    # -- outputs ----------------------------------------------------------------------------------------------------------
    def _out(self, N, parts):
        """A guarded output for ``parts`` [B, H, N, D] tensors -> (buffer, check, pointers, strides, views)."""
        D = self.D
        if self.layout == "bhnd":
            buf, check = kc.guarded((parts, B, H, N, D), F32, self.dev)
            views = [buf[i] for i in range(parts)]
            return buf, check, [t.data_ptr() for t in views], [(H * N * D, N * D, D)] * parts, views
        W = parts * H * D + GAP
        buf, check = kc.guarded((B, N, W), F32, self.dev)
        views = [buf[..., i * H * D:(i + 1) * H * D].view(B, N, H, D).permute(0, 2, 1, 3) for i in range(parts)]
        return buf, check, [buf.data_ptr() + 4 * i * H * D for i in range(parts)], [(N * W, D, W)] * parts, views

    def _gap_intact(self, buf, parts, what):
        if self.layout == "packed":
            gap = buf[..., parts * H * self.D:]
            assert bool((gap == kc.SENTINEL).all()), f"{what}: the gap between rows was written"

    def forward(self, want_lse=True, what=""):
        from makani_amd import ops
        buf, check, ptr, st, views = self._out(self.Nq, 1)
        lse, clse = kc.guarded((B, H, self.Nq), F32, self.dev) if want_lse else (None, None)
        strides = _arr([s for t in self.in_str + st for s in t])
        rc = self.lib.mk_attn_x3_fwd(*self.in_ptr, ptr[0], lse.data_ptr() if want_lse else None, B, H, self.Nq, self.Nk, self.D,
                                     ctypes.addressof(strides), self.scale, ops._stream())
        torch.cuda.synchronize()
        assert rc == 0, self.lib.mk_last_error()
        check(f"{what} o")
        self._gap_intact(buf, 1, f"{what} o")
        if want_lse:
            clse(f"{what} lse")
        self.o_buf, self.o_ptr, self.o_str, self.o, self.lse = buf, ptr[0], st[0], views[0], lse
        return buf, views[0], lse

    def backward(self, what=""):
        """After ``forward``: (buffers of dq, dk, dv, the three views, delta)."""
        from makani_amd import ops
        assert self.Nq == self.Nk or self.layout == "bhnd"
        delta, cdel = kc.guarded((B, H, self.Nq), F32, self.dev)
        st = _arr([s for t in (self.o_str, self.go_str) for s in t])
        rc = self.lib.mk_attn_x3_bwd_delta(self.o_ptr, self.go_ptr, delta.data_ptr(), B, H, self.Nq, self.D, ctypes.addressof(st),
                                           ops._stream())
        assert rc == 0, self.lib.mk_last_error()
        if self.layout == "bhnd":
            dqb, cq, pq, sq, vq = self._out(self.Nq, 1)
            dkb, ck, pk, sk, vk = self._out(self.Nk, 2)
            bufs, checks = (dqb, dkb), (cq, ck)
            ptr, strs, views = pq + pk, sq + sk, vq + vk
        else:
            buf, c, ptr, strs, views = self._out(self.Nq, 3)
            bufs, checks = (buf,), (c,)
        common = self.in_ptr + [self.go_ptr, self.lse.data_ptr(), delta.data_ptr()]
        st = _arr([s for t in self.in_str + [self.go_str, strs[1], strs[2]] for s in t])
        rc = self.lib.mk_attn_x3_bwd_dkv(*common, ptr[1], ptr[2], B, H, self.Nq, self.Nk, self.D, ctypes.addressof(st), self.scale,
                                         ops._stream())
        assert rc == 0, self.lib.mk_last_error()
        st = _arr([s for t in self.in_str + [self.go_str, strs[0]] for s in t])
        rc = self.lib.mk_attn_x3_bwd_dq(*common, ptr[0], B, H, self.Nq, self.Nk, self.D, ctypes.addressof(st), self.scale,
                                        ops._stream())
        torch.cuda.synchronize()
        assert rc == 0, self.lib.mk_last_error()
        cdel(f"{what} delta")
        for c in checks:
            c(f"{what} gradients")
        if self.layout == "packed":
            self._gap_intact(bufs[0], 3, f"{what} dqkv")
        return bufs, views, delta


def _spike(q, k, where):
    """One key whose score exceeds all others by about 30 for every query: a common component in q that only this key has."""
    D = q.shape[-1]
    q, k = q.clone(), k.clone()
    q[..., 0] = 4.0
    k[..., 0] = 0.0
    k[..., where, 0] = 34.0 * math.sqrt(D) / 4.0
    return q, k


def _run_case(dev, D, Nq, Nk, layout, spike=None):
    what = f"D={D} Nq={Nq} Nk={Nk} {layout}" + (f" spike at key {spike}" if spike is not None else "")
    q, k, v, go = xc.make_inputs(Nq, D, 1.0, seed=1, lead=(B, H), Nk=Nk)
    if spike is not None:
        q, k = _spike(q, k, spike)
        s = (q.double() @ k.double().transpose(-1, -2)) / math.sqrt(D)
        others = torch.cat([s[..., :spike], s[..., spike + 1:]], -1).amax(-1)
        gap = s[..., spike] - others
        assert 24 < float(gap.min()) and float(gap.max()) < 40, "the spike is not about 30 above the other scores"
    ref = ac.reference(q, k, v, go)
    pr = Problem(dev, q, k, v, go, layout)
    obuf, o, lse = pr.forward(True, what)
    wf = xc.check("o", o.cpu(), ref, what)
    wl = xc.check("lse", lse.cpu(), ref, what)
    o_keep, lse_keep = obuf.clone(), lse.clone()
    # grad mode off: no lse is stored and the output is unchanged
    obuf0, _, _ = pr.forward(False, what + " (no lse)")
    assert _same_bits(obuf0, o_keep), f"{what}: o differs without lse"
    # backward, on the o and lse of a forward with lse
    obuf1, _, lse1 = pr.forward(True, what + " (second run)")
    assert _same_bits(obuf1, o_keep), f"{what}: o differs between runs"
    assert _same_bits(lse1, lse_keep), f"{what}: lse differs between runs"
    bufs, (dq, dk, dv), delta = pr.backward(what)
    want_delta = (go.double() * o.cpu().double()).sum(-1)
    mag_delta = (go.double().abs() * o.cpu().double().abs()).sum(-1)
    kc.x3_elementwise(delta.cpu(), want_delta, mag_delta, c=kc.F32_C, what=f"{what} delta")      # an fmaf chain over D
    wq, wk, wv = (xc.check(n, t.cpu(), ref, what) for n, t in (("dq", dq), ("dk", dk), ("dv", dv)))
    bufs2, _, delta2 = pr.backward(what + " (second run)")
    assert _same_bits(delta, delta2), f"{what}: delta differs between runs"
    for a, b2 in zip(bufs, bufs2):
        assert _same_bits(a, b2), f"{what}: gradients differ between runs"
    print(f"{what}: o {wf:.3f} lse {wl:.3f} dq {wq:.3f} dk {wk:.3f} dv {wv:.3f} units "
          f"(limits {xc.O_C} {xc.LSE_C} {xc.DQ_C} {xc.DK_C} {xc.DV_C})")


@pytest.mark.parametrize("D,Nq,Nk,layout", _cases(), ids=lambda x: str(x))
def test_attention_every_element(dev, D, Nq, Nk, layout):
    _run_case(dev, D, Nq, Nk, layout)


@pytest.mark.parametrize("D", [48, 64])
@pytest.mark.parametrize("where", ["last", "first"])
def test_attention_spike(dev, D, where):
    """A key about 30 above all others: in the last (ragged) key tile the running maximum moves after accumulation has
    started and everything accumulated is rescaled to nothing; in the first tile every later term underflows."""
    (tq, tk) = _tiles(D)[0]
    n = 2 * max(tq, tk) + 3
    _run_case(dev, D, n, n, "bhnd", spike=(n - 2 if where == "last" else 1))


@pytest.mark.parametrize("bad", ["head_size", "unsupported_head", "stride"])
def test_attention_refuses_without_launching(dev, bad):
    """A head size that is no multiple of 16, one past the supported range and a misaligned token stride: code 1 from every
    entry point, and the outputs keep the sentinel in every element."""
    from makani_amd import _lib, ops
    lib = _lib.load()
    N = 40
    D = {"head_size": 24, "unsupported_head": 80, "stride": 32}[bad]
    sn = D + 2 if bad == "stride" else D
    x = kc.poisoned(torch.randn(B, H, N, 128), dev)
    stat = torch.zeros(B, H, N, dtype=F32, device=dev)
    outs = [kc.guarded((B, H, N, 128), F32, dev) for _ in range(3)]
    lse, clse = kc.guarded((B, H, N), F32, dev)
    st = _arr([H * N * 128, N * 128, sn] * 6)
    sp, s = ctypes.addressof(st), ops._stream()
    xp = x.data_ptr()
    o, dk, dv = (t.data_ptr() for t, _ in outs)
    assert lib.mk_attn_x3_fwd(xp, xp, xp, o, lse.data_ptr(), B, H, N, N, D, sp, 0.25, s) == 1 and lib.mk_last_error()
    assert lib.mk_attn_x3_bwd_delta(xp, xp, lse.data_ptr(), B, H, N, D, sp, s) == 1
    assert lib.mk_attn_x3_bwd_dkv(xp, xp, xp, xp, stat.data_ptr(), stat.data_ptr(), dk, dv, B, H, N, N, D, sp, 0.25, s) == 1
    assert lib.mk_attn_x3_bwd_dq(xp, xp, xp, xp, stat.data_ptr(), stat.data_ptr(), o, B, H, N, N, D, sp, 0.25, s) == 1
    assert (lib.mk_attn_x3_info(D, ctypes.addressof((ctypes.c_int * 6)())) == 1) == (bad != "stride")
    torch.cuda.synchronize()
    for t, c in outs:
        c(bad)
        assert bool((t == kc.SENTINEL).all()), f"{bad}: something was launched"
    clse(bad)
    assert bool((lse == kc.SENTINEL).all())
