"""What the ``*_bench.py`` tools that set a HIP path against its torch formulation share: windows of back-to-back calls between
two device events, the alternating median over such windows, a relative error for the sanity bound before a row is timed, and a
callable that sets a family's ``hip | torch`` variable.  Imported by specattn_bench, specdiag_bench, afno_bench, attn_bench, toknorm_bench,
toklinear_bench, toklinear_fp32_bench, afnov1_bench, patch_bench and rollout_bench; ``bench.py`` at the root has its own timing and does not use it."""
import os

import numpy as np
import torch


def window(fn, calls):
    """``calls`` back-to-back calls between two device events -> seconds per call."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def timed(fns, seconds, rounds):
    """Alternates the callables; per callable the median seconds per call over ``rounds`` windows of >= ``seconds``."""
    calls = []
    for f in fns:
        for _ in range(2):
            f()
        torch.cuda.synchronize()
        est = window(f, 2)
        calls.append(max(2, int(np.ceil(1.1 * seconds / est))))
    out = [[] for _ in fns]
    for _ in range(rounds):
        for f, n, ts in zip(fns, calls, out):
            ts.append(window(f, n))
    return [float(np.median(ts)) for ts in out]


def rel(a, b):
    """|a - b| / |b| in fp32; complex tensors stay as they are."""
    a, b = (a if a.is_complex() else a.float()), (b if b.is_complex() else b.float())
    return (torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b)).item()


def with_knob(env, value, fn):
    def run():
        os.environ[env] = value        # read at call time
        return fn()
    return run
