"""Optimizer step on the north-star parameter set (sfno_linear_73chq_sc3_layers8_edim384), one process, alternating:
FusedAdam, FusedAdamW (without / with max_grad_norm), FusedLAMB and torch.optim.AdamW(fused=True), timed with device
events after warm-up; ms per step and GB/s against the algorithmic bytes per real.  Then one whole training step
(forward + loss + backward + clip + AdamW) replayed as one graph against the same step run eagerly.

    python tools/optim_bench.py [--quick] [--steps K] [--rounds R]

--quick: 3 steps of each optimizer and no whole-step part (for a kernel trace: rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import CONFIG  # noqa: E402
from makani_amd.optim import FusedAdam, FusedAdamW, FusedLAMB, clip_grad_norm_  # noqa: E402
from makani_amd.sfnonet import SphericalFourierNeuralOperatorNet  # noqa: E402

BYTES = {"FusedAdam": 28, "FusedAdamW": 28, "FusedAdamW+clip": 32, "FusedLAMB": 44, "torch AdamW fused": 28}


def time_steps(fn, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(333)
    net = SphericalFourierNeuralOperatorNet(**CONFIG).to(dev)
    params = [p for p in net.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    reals = sum(p.numel() * (2 if p.is_complex() else 1) for p in params)
    # torch's fused AdamW on real views (detached leaves sharing the storage)
    tviews = []
    for p in params:
        v = (torch.view_as_real(p.data) if p.is_complex() else p.data).detach()
        v.grad = torch.view_as_real(p.grad) if p.is_complex() else p.grad
        tviews.append(v)
    opts = {"FusedAdam": FusedAdam(params, lr=1e-6),
            "FusedAdamW": FusedAdamW(params, lr=1e-6, betas=(0.9, 0.95)),
            "FusedAdamW+clip": FusedAdamW(params, lr=1e-6, betas=(0.9, 0.95), max_grad_norm=32.0),
            "FusedLAMB": FusedLAMB(params, lr=1e-6),
            "torch AdamW fused": torch.optim.AdamW(tviews, lr=1e-6, fused=True)}
    print(f"{len(params)} tensors, {reals / 1e6:.1f} M reals", flush=True)
    k = 3 if args.quick else args.steps
    rounds = 1 if args.quick else args.rounds
    for o in opts.values():          # warm-up (state allocation, plans)
        o.step()
    torch.cuda.synchronize()
    times = {n: [] for n in opts}
    for _ in range(rounds):
        for n, o in opts.items():
            times[n].append(time_steps(o.step, k))
    base = statistics.median(times["FusedAdam"])
    res = {}
    for n, ts in times.items():
        ms = statistics.median(ts)
        res[n] = dict(ms=round(ms, 3), rel_to_FusedAdam=round(ms / base, 3),
                      GBps=round(BYTES[n] * reals / ms / 1e6, 1), bytes_per_real=BYTES[n])
        print(f"{n:20s} {ms:8.3f} ms  x{ms / base:5.3f}  {BYTES[n] * reals / ms / 1e6:8.1f} GB/s "
              f"({BYTES[n]} B/real)", flush=True)
    if args.quick:
        print(json.dumps({"optimizers": res}))
        return
    del opts, tviews
    for p in params:
        p.grad = None
    torch.cuda.empty_cache()

    # whole step: forward + loss + backward + clip + AdamW, eager vs one graph replay
    inp = torch.randn(1, CONFIG["inp_chans"], *CONFIG["inp_shape"], device=dev)
    tar = torch.randn(1, CONFIG["out_chans"], *CONFIG["out_shape"], device=dev)
    opt = FusedAdamW(params, lr=1e-6, betas=(0.9, 0.95), max_grad_norm=32.0, capturable=True)

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = ((net(inp).float() - tar) ** 2).mean()
        loss.backward()
        clip_grad_norm_(params, 32.0)
        opt.step()

    def eager():
        net.zero_grad(set_to_none=True)
        step()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            eager()
        s.synchronize()
        te = [time_steps(eager, 5) for _ in range(3)]
        net.zero_grad(set_to_none=True)
        g = torch.cuda.CUDAGraph()
        g.capture_begin()
        step()
        g.capture_end()
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    tg = [time_steps(g.replay, 5) for _ in range(3)]
    res["whole_step"] = dict(eager_ms=round(statistics.median(te), 2), graph_ms=round(statistics.median(tg), 2))
    print(f"whole step (fwd + loss + bwd + clip_grad_norm_ + FusedAdamW max_grad_norm): eager "
          f"{statistics.median(te):.2f} ms, one graph replay {statistics.median(tg):.2f} ms", flush=True)
    print(json.dumps({"optimizers": res}))


if __name__ == "__main__":
    main()
