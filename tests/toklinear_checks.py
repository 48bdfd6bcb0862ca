"""Bounds for the token-major linear kernels (csrc/toklinear.hip), shared by tests/test_toklinear_gpu.py and the checker's own
test in tests/test_toklinear_cpu.py (a plain module, not a conftest).

All references are float64 on the bf16-rounded operands.  The forward bounds are ``kernel_checks.bf16_elementwise`` with
``gamma = gemm_gamma`` of the two operands (the fp32 accumulation of exact products, any order):

* plain output ``bf16(acc + b)``: ``slack_plain(gamma)``;
* pre-activation ``bf16(acc + b)``: ``slack_pre(gamma, pre64)``;
* ``act``: against ``gelu64`` of the STORED ``pre``, one ulp plus ``2^-23 |act|`` -- a wrong ``pre`` is caught once, by the
  check of the pre-activation;
* addend mode: the fp32 output minus the addend against the bf16 bound of ``acc + b``, plus ``2^-23 (|addend| + |out|)`` for
  the one fp32 addition;
* GELU' mode ``bf16(acc gelu'(aux))``: ``slack_aux(gamma)``.

Weight gradient (fp32 sums of exact products over R tokens, any order, here slabs added in order):
``|dW - ref| <= R 2^-23 (|dY|^T @ |X|) + 2^-24 |ref|``; ``db`` the same with ``|dY|`` summed over the rows."""
import torch

import kernel_checks as kc


class Ref:
    """float64 ``acc = x w^T``, ``pre = acc + b`` and ``gamma`` for bf16 ``x`` ``[R, I]``, ``w`` ``[O, I]``, fp32 ``b`` ``[O]`` or None."""

    def __init__(self, x, w, b=None):
        x64, w64 = x.double().cpu(), w.double().cpu()
        self.acc = x64 @ w64.T
        self.pre = self.acc if b is None else self.acc + b.double().cpu()
        self.gamma = kc.gemm_gamma(x64, w64.T)


def check_plain(y, ref, what=""):
    return kc.bf16_elementwise(y, ref.pre, kc.slack_plain(ref.gamma), what)


def check_pre(pre, ref, what=""):
    return kc.bf16_elementwise(pre, ref.pre, kc.slack_pre(ref.gamma, ref.pre), what)


def check_act(act, pre_stored, what=""):
    want = kc.gelu64(pre_stored.double().cpu())
    return kc.bf16_elementwise(act, want, 2.0 ** -23 * want.abs(), what)


def check_addend(out, addend, ref, what=""):
    out64, add64 = out.double().cpu(), addend.double().cpu()
    slack = kc.slack_pre(ref.gamma, ref.pre) + 2.0 ** -23 * (add64.abs() + out64.abs())
    return kc.bf16_elementwise(out64 - add64, ref.pre, slack, what)


def check_aux(y, ref, aux, what=""):
    return kc.bf16_elementwise(y, ref.acc * kc.gelu_grad64(aux.double().cpu()), kc.slack_aux(ref.gamma), what)


def _fp32_sum_check(got, ref64, mag64, R, what):
    got = got.double().cpu()
    assert tuple(got.shape) == tuple(ref64.shape), f"{what}: shape {tuple(got.shape)} against {tuple(ref64.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: NaN or Inf"
    bound = R * 2.0 ** -23 * mag64 + 2.0 ** -24 * ref64.abs()
    err = (got - ref64).abs()
    bad = err > bound
    if bool(bad.any()):
        ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        flat = int(torch.argmax(ratio))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements exceed the bound, the worst |got - ref| / bound = "
                             f"{float(ratio.flatten()[flat]):.3f} at flat index {flat}")
    safe = torch.where(bound > 0, bound, torch.ones_like(bound))
    return float((err / safe).max())


def check_wgrad(dw, dy, x, what=""):
    """``dw`` fp32 ``[O, I]`` against ``dy^T x`` of bf16 ``dy`` ``[R, O]`` and ``x`` ``[R, I]``."""
    dy64, x64 = dy.double().cpu(), x.double().cpu()
    return _fp32_sum_check(dw, dy64.T @ x64, dy64.abs().T @ x64.abs(), dy.shape[0], what)


def check_dbias(db, dy, what=""):
    dy64 = dy.double().cpu()
    return _fp32_sum_check(db, dy64.sum(0), dy64.abs().sum(0), dy.shape[0], what)


# ---- the stated arithmetic, evaluated exactly with its rounding points (float64 between them) ---------------------------------
def emulate_plain(ref):
    return ref.pre.to(torch.bfloat16)


def emulate_act(pre_bf16):
    return kc.gelu64(pre_bf16.double()).to(torch.bfloat16)


def emulate_addend(ref, addend):
    return (addend.double() + ref.pre.to(torch.bfloat16).double()).float()


def emulate_aux(ref, aux):
    return (ref.acc * kc.gelu_grad64(aux.double())).to(torch.bfloat16)
