#!/usr/bin/env python3
"""Times the one-pass input assembly (csrc/preproc.hip) against the torch formulation of the reference on one MI355X.

    python3 tools/stepper_bench.py [--iters 20] [--warmup 5] [--out FILE.json]

Shapes of the reference's configs: 73 predicted + 1 unpredicted + 35 static channels at 721 x 1440, B in {1, 2},
output fp32 and bf16 (the torch side includes the ``.to(bfloat16)`` the net would do), history normalisation "none" and
"exponential".  ``Preprocessor2D.assemble`` (HIP) and ``Preprocessor2D._assemble_torch`` (concat, tile, concat, mask,
cast; in mode "exponential" float64 raw sums in torch ops) run on the same inputs, alternated, each timed with device
events.  ``mk_history_sums`` and ``mk_input_assemble_bwd`` are timed alone.  Before anything is timed the tool asserts,
at the timed size, that the two paths agree bit for bit (mode "none") / that the HIP field is torch's arithmetic on the
kernel's own statistics (mode "exponential").  It fails when no GPU is found.

Per case: median and 10th-90th percentile in ms, the algorithmic bytes computed from the shapes (every source read
once, the output written once; the statistics modes read the history twice) and the achieved bytes/s of the HIP path,
to be read next to the measured copy ceiling of this access pattern, 4.5-5.3 TB/s (profiles/r02_membench.txt).  Run the
command twice and compare: the spread between two runs is part of the result.  Kernel names are stable
(input_assemble_kernel, input_assemble_bwd_kernel, history_sums_kernel, history_finalize), so a separate
``rocprofv3 --kernel-trace --stats -- python3 tools/stepper_bench.py`` attributes them.
"""
import argparse
import json
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C, CU, CS, H, W = 73, 1, 35, 721, 1440
CEILING_TBS = (4.5, 5.3)


def make_preprocessor(tmp, mode, dev):
    from makani_amd.preprocessor import Preprocessor2D
    g = torch.Generator().manual_seed(1)
    oro, lsm = os.path.join(tmp, "oro.npy"), os.path.join(tmp, "lsm.npy")
    if not os.path.exists(oro):
        np.save(oro, (3000.0 * torch.rand(H, W, generator=g)).numpy())
        np.save(lsm, (torch.rand(H, W, generator=g) > 0.6).numpy().astype(np.int64))
    p = SimpleNamespace(n_history=0, history_normalization_mode=mode, history_normalization_decay=0.5, target="default",
                        normalize_residual=False, img_shape_x=H, img_shape_y=W, img_local_offset_x=0, img_local_offset_y=0,
                        img_local_shape_x=H, img_local_shape_y=W, add_grid=True, gridtype="sinusoidal", grid_num_frequencies=16,
                        add_orography=True, orography_path=oro, add_landmask=True, landmask_path=lsm, n_future=0,
                        masked_channels=[20])
    pp = Preprocessor2D(p).to(dev)
    pp.eval()
    assert pp.static_features.shape[1] == CS
    return pp


def timed(fns, iters, warmup):
    """Alternates the callables; returns per callable the list of device-event times in ms."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(iters):
        for f, ts in zip(fns, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
    return times


def stats(ts):
    q = np.percentile(np.asarray(ts), [50, 10, 90])
    return dict(median_ms=round(float(q[0]), 4), p10_ms=round(float(q[1]), 4), p90_ms=round(float(q[2]), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stepper_bench: no GPU found")
    from makani_amd import _lib, ops
    dev = torch.device("cuda:0")
    lib = _lib.load()
    results = []
    hw4 = H * W * 4
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
        for mode in ("none", "exponential"):
            pp = make_preprocessor(tmp, mode, dev)
            for B in (1, 2):
                g = torch.Generator(device=dev).manual_seed(B)
                x = torch.randn(B, C, H, W, device=dev, generator=g) * 2.0 + 1.0
                u = torch.rand(B, 1, CU, H, W, device=dev, generator=g)
                pp.unpredicted_inp_eval = None
                pp.cache_unpredicted_features(None, None, u, None)
                # correctness at the timed size, before any timing
                got = pp.assemble(x)
                if mode == "none":
                    assert torch.equal(got, pp._assemble_torch(x)), "HIP and torch assembly differ"
                else:
                    xa = torch.cat([x.unsqueeze(1), u], dim=2)
                    want = ((xa - pp.history_mean.unsqueeze(1)) / pp.history_std.unsqueeze(1)).reshape(B, C + CU, H, W)
                    want[:, 20] *= pp.static_features[0, -1]
                    assert torch.equal(got[:, :C + CU], want), "HIP field is not torch's arithmetic on its statistics"
                    del xa, want
                assert torch.equal(pp.assemble(x, torch.bfloat16), got.to(torch.bfloat16)), "bf16 output is not the rounded fp32 output"
                del got
                src = B * (C + CU) * hw4
                for od, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
                    nbytes = src * (2 if mode != "none" else 1) + CS * hw4 + B * (C + CU + CS) * H * W * (4 if od == torch.float32 else 2)
                    t_hip, t_torch = timed([lambda: pp.assemble(x, od), lambda: pp._assemble_torch(x, od)], args.iters, args.warmup)
                    r = dict(case="assemble", mode=mode, B=B, out=name, bytes=nbytes, hip=stats(t_hip), torch=stats(t_torch))
                    r["hip_TBs"] = round(nbytes / (r["hip"]["median_ms"] * 1e-3) / 1e12, 3)
                    r["speedup"] = round(r["torch"]["median_ms"] / r["hip"]["median_ms"], 2)
                    results.append(r)
                    print(json.dumps(r), flush=True)
                # the statistics pass and the backward pass alone
                x5 = x.unsqueeze(1)
                wt = torch.ones(1, device=dev)
                (t_sum,) = timed([lambda: ops.history_sums(x5, u, wt)], args.iters, args.warmup)
                r = dict(case="mk_history_sums", mode=mode, B=B, bytes=src, hip=stats(t_sum))
                r["hip_TBs"] = round(src / (r["hip"]["median_ms"] * 1e-3) / 1e12, 3)
                results.append(r)
                print(json.dumps(r), flush=True)
                if mode == "none":
                    for gd, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
                        gout = torch.randn(B, C + CU + CS, H, W, device=dev, generator=g).to(gd)
                        gx = torch.empty(B, 1, C, H, W, device=dev)
                        mask = pp._masked_outputs(C + CU, dev)[1]
                        stat = pp.static_features[0]

                        def bwd():
                            _lib.check(lib.mk_input_assemble_bwd(gout.data_ptr(), 0 if gd == torch.float32 else 1, stat.data_ptr(), None,
                                                                 mask.data_ptr(), mask.numel(), CS - 1, gx.data_ptr(), 0, B, 1, C, CU, CS,
                                                                 H, W, torch.cuda.current_stream().cuda_stream))

                        (t_bwd,) = timed([bwd], args.iters, args.warmup)
                        nbytes = B * C * H * W * ((4 if gd == torch.float32 else 2) + 4)
                        r = dict(case="mk_input_assemble_bwd", B=B, gout=name, bytes=nbytes, hip=stats(t_bwd))
                        r["hip_TBs"] = round(nbytes / (r["hip"]["median_ms"] * 1e-3) / 1e12, 3)
                        results.append(r)
                        print(json.dumps(r), flush=True)
                        del gout, gx
                del x, u
                torch.cuda.empty_cache()
    summary = dict(tool="stepper_bench", shape=[C, CU, CS, H, W], iters=args.iters, copy_ceiling_TBs=list(CEILING_TBS), results=results)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
    print("stepper_bench: done")


if __name__ == "__main__":
    main()
