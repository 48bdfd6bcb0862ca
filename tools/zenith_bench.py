#!/usr/bin/env python3
"""Times the zenith kernel (csrc/zenith.hip) on one MI355X against the two other ways to get the channel.

    python3 tools/zenith_bench.py [--iters 20] [--warmup 5] [--reps 10] [--out FILE.json]

At 721 x 1440 for n = 2, 16 and 80 time levels (8.3, 66 and 332 MB; the last does not fit the 256 MiB Infinity Cache,
so back-to-back rewrites of it have to reach HBM):

* ``kernel``: ``mk_cos_zenith`` through the C ABI into a preallocated output (one launch of ``cos_zenith_kernel``);
* ``module``: ``CosZenith.forward`` (``ops.cos_zenith``: the output's allocation, the argument checks and the launch);
* ``torch``: the broadcast formulation in torch ops on the device (``CosZenith(..., use_hip=False)``);
* ``fill``: ``out.fill_(1.0)``, torch's own store-only kernel on the same buffer, the store rate to read ``kernel`` against;
* ``host``: the route the reference prescribes -- ``zenith.cos_zenith_angle`` in numpy on the host plus the copy to the
  device, timed end to end with the wall clock around a synchronise.

The device paths are alternated and timed with device events.  One call lasts 8-40 us, less than the host needs to issue
it, so an event pair around a single call would time the host: a sample is ``--reps`` calls back to back between one pair
of events, divided by ``--reps``.

Before anything is timed the tool asserts at the timed size that the kernel is within 2 x ``pixel_rounding`` (read from
tests/golden/ref_zenith.npz) of the numpy function and that two launches agree bit for bit.  Per case: median and
10th-90th percentile in ms per call, the bytes written and the kernel's bytes per second.  Run the command twice and compare: the
spread between two runs is part of the result.  ``MK_LIB_OVERRIDE`` selects an A/B build of the library.  It fails when
no GPU is found.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 721, 1440


def timed(fns, iters, warmup, reps):
    """Alternates the callables; returns per callable the list of device-event times in ms per call, each the mean over
    ``reps`` calls issued back to back."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(iters):
        for f, ts in zip(fns, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                f()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) / reps)
    return times


def stats(ts):
    q = np.percentile(np.asarray(ts), [50, 10, 90])
    return dict(median_ms=round(float(q[0]), 4), p10_ms=round(float(q[1]), 4), p90_ms=round(float(q[2]), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("zenith_bench: no GPU found")
    from makani_amd import _lib, ops, zenith
    dev = torch.device("cuda:0")
    lib = _lib.load()
    bound = 2.0 * float(np.load(os.path.join(ROOT, "tests", "golden", "ref_zenith.npz"))["pixel_rounding"])
    lat, lon = zenith.default_grid(H, W)
    lon2, lat2 = np.meshgrid(lon, lat)
    mod = zenith.CosZenith(lat, lon).to(dev)
    results = []
    with torch.no_grad():
        for n in (2, 16, 80):
            times = (np.datetime64("2018-03-21T06:00", "us") + np.arange(n) * np.timedelta64(6, "h"))
            eph = torch.from_numpy(zenith.solar_ephemeris(times)).to(dev)
            out = torch.empty(n, H, W, device=dev)

            def hip():
                _lib.check(lib.mk_cos_zenith(eph.data_ptr(), mod.sin_lat.data_ptr(), mod.cos_lat.data_ptr(), mod.lon_rad.data_ptr(),
                                             out.data_ptr(), n, H, W, torch.cuda.current_stream().cuda_stream), "mk_cos_zenith")

            def host():
                return torch.from_numpy(zenith.cos_zenith_angle(times, lon2, lat2)).to(dev)

            # correctness at the timed size, before any timing
            hip()
            first = out.clone()
            hip()
            assert torch.equal(out, first), "two launches differ"
            err = float((out.double() - host().double()).abs().max())
            assert err <= bound, f"kernel is {err:.3e} from the numpy function (bound {bound:.3e})"
            del first
            nbytes = n * H * W * 4
            assert torch.equal(mod(eph[None])[0, :, 0], out), "the module is not the kernel"
            t_hip, t_mod, t_torch, t_fill = timed([hip, lambda: mod(eph[None]), lambda: mod(eph[None], use_hip=False),
                                                   lambda: out.fill_(1.0)], args.iters, args.warmup, args.reps)
            t_host = []
            for k in range(args.warmup + args.iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host()
                torch.cuda.synchronize()
                if k >= args.warmup:
                    t_host.append((time.perf_counter() - t0) * 1e3)
            r = dict(case="cos_zenith", n=n, bytes=nbytes, max_err_vs_numpy=err, kernel=stats(t_hip), module=stats(t_mod),
                     torch=stats(t_torch), fill=stats(t_fill), host=stats(t_host))
            r["kernel_TBs"] = round(nbytes / (r["kernel"]["median_ms"] * 1e-3) / 1e12, 3)
            r["fill_TBs"] = round(nbytes / (r["fill"]["median_ms"] * 1e-3) / 1e12, 3)
            r["speedup_vs_torch"] = round(r["torch"]["median_ms"] / r["kernel"]["median_ms"], 2)
            r["speedup_vs_host"] = round(r["host"]["median_ms"] / r["kernel"]["median_ms"], 1)
            results.append(r)
            print(json.dumps(r), flush=True)
            del out
    summary = dict(tool="zenith_bench", shape=[H, W], iters=args.iters, reps=args.reps, lib=os.environ.get("MK_LIB_OVERRIDE", "default"),
                   results=results)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
    print("zenith_bench: done")


if __name__ == "__main__":
    main()
