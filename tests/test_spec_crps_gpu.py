"""GPU tests of ``mk_spec_crps_sums`` / ``mk_spec_crps_bwd`` (csrc/spec_crps.hip) through the C ABI -- guarded outputs, poisoned
inputs, the unstored triangle full of NaN, the guard bands compared bit for bit after every launch -- against the references
and bounds of tests/spec_crps_checks.py; of ``ops.spectral_crps_sums`` behind ``EnsembleSpectralCRPSLoss`` on the 33 x 64 grid
against the torch formulation on the device; and of a captured forward + backward."""
import numpy as np
import pytest
import torch

import capi_checks as capi
import spec_crps_checks as sc
from kernel_checks import guarded, node_kinds, poisoned, row_rel
from test_spec_crps_cpu import REFUSED

pytestmark = pytest.mark.gpu

# (L, M, B, E, C), l_off, m_off: the smallest; two chunks of 16 orders and a ragged tail of 5, B C = 6 no multiple of a wave; the
# most members; B C = 73 beyond a wave; shards: degrees from 3 on, orders from 5 on (rows with nothing stored, no order of
# weight 1), both offsets
WHOLE = [((5, 5, 1, 2, 1), 0, 0), ((40, 37, 2, 3, 3), 0, 0), ((9, 4, 1, 16, 2), 0, 0), ((7, 7, 1, 5, 73), 0, 0)]
SHARDS = [((8, 6, 2, 4, 3), 3, 0), ((8, 6, 2, 4, 3), 0, 5), ((8, 6, 2, 4, 3), 2, 2)]
ids = lambda c: "x".join(map(str, c[0])) + f"@{c[1]},{c[2]}"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def launch_sums(dev, cp, ct, dims, l_off=0, m_off=0):
    """One call of mk_spec_crps_sums on numpy spectra between NaN bands: S ``[B C, L, 2]`` as numpy, after the band checks of
    the output and of the workspace."""
    from makani_amd import _lib
    lib = _lib.load()
    L, M, B, E, C = dims
    pd, td = poisoned(torch.from_numpy(np.array(cp)), dev), poisoned(torch.from_numpy(np.array(ct)), dev)
    n = lib.mk_spec_crps_workspace(L, M, B * C)
    assert n >= 2 * L * B * C
    ws, check_ws = guarded((n,), torch.float64, dev)
    out, check = guarded((L, B * C, 2), torch.float64, dev)
    _lib.check(lib.mk_spec_crps_sums(pd.data_ptr(), td.data_ptr(), ws.data_ptr(), out.data_ptr(), L, M, B, E, C, l_off, m_off,
                                     _stream()), "mk_spec_crps_sums")
    torch.cuda.synchronize()
    check("S")
    check_ws("workspace")
    return out.cpu().permute(1, 0, 2).contiguous().numpy()


def launch_bwd(dev, cp, ct, gs, dims, l_off=0, m_off=0):
    """One call of mk_spec_crps_bwd: the gradient ``[L, M, B E C]`` complex64 as numpy, after the band check."""
    from makani_amd import _lib
    lib = _lib.load()
    L, M, B, E, C = dims
    pd, td = poisoned(torch.from_numpy(np.array(cp)), dev), poisoned(torch.from_numpy(np.array(ct)), dev)
    gd = poisoned(torch.from_numpy(np.array(np.transpose(gs, (1, 0, 2)), order="C")), dev)      # [L, B C, 2], as the kernel wrote S
    out, check = guarded((L, M, B * E * C), torch.complex64, dev)
    _lib.check(lib.mk_spec_crps_bwd(pd.data_ptr(), td.data_ptr(), gd.data_ptr(), out.data_ptr(), L, M, B, E, C, l_off, m_off,
                                    _stream()), "mk_spec_crps_bwd")
    torch.cuda.synchronize()
    check("gradient")
    return out.cpu().numpy()


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("case", WHOLE + SHARDS, ids=ids)
def test_sums_and_gradient_against_the_reference(dev, case, kind):
    dims, l_off, m_off = case
    cp, ct, gs = sc.problem(dims, kind, l_off, m_off)
    what = f"{ids(case)} {kind}"
    sc.assert_sums(launch_sums(dev, cp, ct, dims, l_off, m_off), cp, ct, dims, l_off, m_off, what)
    got = launch_bwd(dev, cp, ct, gs, dims, l_off, m_off)
    sc.assert_grad(got, cp, ct, gs, dims, l_off, m_off, what)
    if kind == "nan":
        points = set(p for p, _ in sc.nan_points(dims, l_off, m_off))
        assert int(np.isnan(got.real).sum()) == int(np.isnan(got.imag).sum()) == dims[3] * len(points)


def test_rows_of_an_l_slice_carry_the_bits_of_the_whole(dev):
    dims = (40, 37, 2, 3, 3)
    cp, ct, gs = sc.problem(dims, "nan")
    whole, gwhole = launch_sums(dev, cp, ct, dims), launch_bwd(dev, cp, ct, gs, dims)
    for l0, l1 in ((0, 13), (13, 40)):
        sub = (l1 - l0,) + dims[1:]
        part = launch_sums(dev, cp[l0:l1], ct[l0:l1], sub, l_off=l0)
        assert np.array_equal(part.view(np.int64), whole[:, l0:l1].copy().view(np.int64)), (l0, l1)
        gpart = launch_bwd(dev, cp[l0:l1], ct[l0:l1], gs[:, l0:l1], sub, l_off=l0)
        assert np.array_equal(gpart.view(np.int32), gwhole[l0:l1].copy().view(np.int32)), (l0, l1)


def test_m_slices_add_up(dev):
    """Two shards of the orders: their sums add up to the whole within the sum of their bounds plus one rounding of the addition."""
    dims = (40, 37, 2, 3, 3)
    L, M, B, E, C = dims
    cp, ct, _ = sc.problem(dims, "normal")
    want = sc.sums(cp, ct, dims)
    total, lim = np.zeros_like(want), sc.U * np.abs(want)
    for m0, m1 in ((0, 21), (21, 37)):
        sub = (L, m1 - m0, B, E, C)
        part = launch_sums(dev, np.ascontiguousarray(cp[:, m0:m1]), np.ascontiguousarray(ct[:, m0:m1]), sub, m_off=m0)
        pw = sc.sums(cp[:, m0:m1], ct[:, m0:m1], sub, m_off=m0)
        sc.assert_sums(part, cp[:, m0:m1], ct[:, m0:m1], sub, 0, m0, f"orders {m0} ... {m1 - 1}", want=pw)
        total += part
        lim += sc.bound(pw, sub, 0, m0)
    assert (np.abs(total - want) <= lim).all()


def test_two_launches_give_the_same_bits(dev):
    dims = (40, 37, 2, 3, 3)
    cp, ct, gs = sc.problem(dims, "nan")
    a, b = (launch_sums(dev, cp, ct, dims) for _ in range(2))
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    a, b = (launch_bwd(dev, cp, ct, gs, dims) for _ in range(2))
    assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("case", REFUSED, ids=capi.case_ids(REFUSED))
def test_bad_argument_is_refused_and_launches_nothing(dev, case):
    """E = 1, E = 17, a misaligned or null pointer, bad sizes: code 1 and the message; the addresses are never dereferenced (a
    launch on them would fault), and the device still answers afterwards."""
    capi.assert_refused(*case)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- the module on the 33 x 64 grid, capture
H, W = 33, 64


def _fields(dev, B, E, C, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    tar = torch.randn(B, C, H, W, generator=gen)
    prd = tar.repeat_interleave(E, dim=0) + 0.5 * torch.randn(B * E, C, H, W, generator=gen)
    return prd.to(dev, dtype), tar.to(dev)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("B,E,C", [(1, 3, 2), (2, 4, 3)])
def test_module_against_the_torch_formulation_on_the_device(dev, monkeypatch, B, E, C, dtype):
    """Both paths read the same spectra (the transform does not depend on the switch): the loss within one fp32 ulp, ``prd.grad``
    within 1e-5 relative L2 per row (the fp32 transform's backward of gradients that differ by one fp32 rounding)."""
    from makani_amd.ensemble import EnsembleSpectralCRPSLoss
    loss = EnsembleSpectralCRPSLoss((H, W), E, alpha=1.0).to(dev)
    prd, tar = _fields(dev, B, E, C, dtype, 3)
    chw = torch.linspace(0.5, 1.5, C, device=dev).reshape(1, C)
    res = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_SPEC_CRPS", mode)
        x = prd.clone().requires_grad_(True)
        out = loss(x, tar, chw)
        assert ("_SpecCrpsSumsBackward" in node_kinds(out)) == (mode == "hip")
        assert out.dtype == torch.float32 and loss.last_degree_sums.shape == (B, C, loss.sht.lmax, 2)
        out.backward()
        torch.cuda.synchronize()
        assert x.grad.dtype == dtype and x.grad.shape == x.shape
        res[mode] = (float(out.detach()), x.grad.double().cpu().numpy(), loss.last_degree_sums.cpu().numpy())
    (lh, gh, dh), (lt, gt, dt) = res["hip"], res["torch"]
    print(f"B={B} E={E} C={C} {dtype}: loss hip {lh!r} torch {lt!r}")
    assert lh > 0 and abs(lh - lt) <= float(np.spacing(np.float32(abs(lt))))
    assert np.allclose(dh, dt, rtol=1e-12, atol=0)
    rel = row_rel(gh, gt)
    print(f"  prd.grad: worst relative L2 of a row {rel.max():.2e}")
    assert rel.max() <= 1e-5
    with pytest.raises(ValueError, match="expected"):
        loss(prd[..., :-1, :], tar[..., :-1, :], chw)


def test_captured_forward_and_backward_replay_to_the_eager_bits(dev, monkeypatch):
    from makani_amd.ensemble import EnsembleSpectralCRPSLoss
    monkeypatch.setenv("MK_SPEC_CRPS", "hip")
    B, E, C = 2, 4, 3
    loss = EnsembleSpectralCRPSLoss((H, W), E, alpha=0.95).to(dev)
    chw = torch.linspace(0.5, 1.5, C, device=dev).reshape(1, C)
    fresh = [_fields(dev, B, E, C, torch.float32, seed) for seed in (5, 6)]

    def step(x, t):
        out = loss(x, t, chw)
        out.backward()
        return out.detach()

    eager = []
    for p, t in fresh:
        x = p.clone().requires_grad_(True)
        eager.append((step(x, t).clone(), x.grad.clone()))
    x = torch.zeros(B * E, C, H, W, device=dev).requires_grad_(True)
    t = torch.zeros(B, C, H, W, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(x, t)                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(x, t)
    for (p, tt), (l_want, g_want) in zip(fresh, eager):
        with torch.no_grad():
            x.copy_(p)
            t.copy_(tt)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), l_want.view(torch.int32))
        assert torch.equal(x.grad.view(torch.int32), g_want.view(torch.int32))
