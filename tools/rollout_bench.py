#!/usr/bin/env python3
"""Times the rollout tail (csrc/rollout.hip) and a whole rollout through ``makani_amd.inference.Rollout`` on one MI355X.

    python3 tools/rollout_bench.py [--window 0.1] [--rounds 3] [--part tail,kernel,rollout] [--steps 20] [--out FILE.json]

At 73 x 721 x 1440 for B = 1 and 2, fp32 and bf16 model output:

* the tail alone, ``MK_ROLLOUT=hip`` against ``MK_ROLLOUT=torch`` (``ops.rollout_tail`` on the same inputs, alternated in one
  process), in three variants: denormalise + score + map; plus mask and hold; plus the emit of all channels;
* the kernel against its algorithmic bytes in TB/s (every stream that the variant reads or writes counted once: the model
  output, the prediction, the target, the climatology and the map twice -- read and written --, the last input step for the
  held channel and the mask for the masked one, the emitted fields);
* a ``--steps``-step scored rollout of the ``bench.py`` SFNO configuration under bf16 autocast through ``Rollout``
  (``MK_ROLLOUT=hip``) against the same loop written with ``SingleStepWrapper`` and torch ops (held channel, loss,
  ``MetricsHandler.update``, squared-error map and curve, channel selection and de-normalisation, copy to the host).

Each sample is a window of back-to-back calls between one pair of device events, sized from a warm-up estimate to last at
least ``--window`` seconds; per row the median over ``--rounds`` windows (``event_timing.py``).  Before a row is timed the two
paths are compared on its inputs.  It fails when no GPU is found.  The default of ``MK_ROLLOUT`` follows DESIGN section 19:
``hip`` only if no row here is slower than the torch path; the table of DESIGN section 34 is this tool's output.
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from event_timing import rel, timed, window, with_knob  # noqa: E402

C, H, W = 73, 721, 1440
MASKED, HELD = 20, 20


def tail_inputs(dev, B, dtype):
    g = torch.Generator(device=dev).manual_seed(B)
    r = lambda *s: torch.rand(*s, device=dev, generator=g)
    clim = 0.5 * torch.randn(C, H, W, device=dev, generator=g)
    tar = clim + torch.randn(B, C, H, W, device=dev, generator=g)
    yn = (0.8 * tar + 0.4 * torch.randn(B, C, H, W, device=dev, generator=g)).to(dtype)
    return dict(yn=yn, tar=tar, clim=clim, wrow=r(H) + 0.1, mean=0.1 * r(B, C), std=0.9 + 0.2 * r(B, C), mask=r(H, W),
                x_last=0.5 * tar, err=torch.zeros(C, H, W, device=dev), escale=1.0 + r(C), eshift=r(C))


def variants(t, dev):
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    base = dict(mean=t["mean"], std=t["std"], tar=t["tar"], clim=t["clim"], wrow=t["wrow"], err_map=t["err"])
    held = dict(base, mask=t["mask"], mask_chans=i32([MASKED]), x_last=t["x_last"], hold_chans=i32([HELD]))
    emit = dict(held, emit_chans=i32(list(range(C))), emit_scale=t["escale"], emit_shift=t["eshift"])
    return [("denorm + score + map", base), ("+ mask and hold", held), ("+ emit of all channels", emit)]


def algorithmic_bytes(B, dtype, kw):
    field = H * W * 4
    n = B * C * H * W * (4 if dtype == torch.float32 else 2)        # the model output
    n += B * C * field * 2                                          # the prediction written, the target read
    n += C * field * 3                                              # the climatology read, the map read and written
    if "mask_chans" in kw:
        n += field + B * field                                      # the mask for one channel, the last input step for one
    if "emit_chans" in kw:
        n += B * C * field
    return n


def make_params(steps, held):
    return SimpleNamespace(n_history=0, history_normalization_mode="exponential", history_normalization_decay=0.5, target="default",
                           normalize_residual=False, img_shape_x=H, img_shape_y=W, img_local_offset_x=0, img_local_offset_y=0,
                           img_local_shape_x=H, img_local_shape_y=W, add_grid=False, add_orography=False, add_landmask=False,
                           n_future=0, held_channels=held, log_to_screen=False, log_to_wandb=False,
                           channel_names=["u10m", "t2m", "z500"] + [f"c{i}" for i in range(C - 3)], dt=1, dhours=6,
                           split_data_channels=False, valid_autoreg_steps=steps - 1, N_out_channels=C, img_crop_shape_x=H,
                           img_crop_shape_y=W, img_crop_offset_x=0, img_crop_offset_y=0, model_grid_type="equiangular",
                           loss="geometric l2", channel_weights="auto")


def rollout_rows(dev, steps, args, rows):
    """A scored rollout of the bench.py SFNO through Rollout against the loop written by hand."""
    import bench
    from makani_amd.inference import Rollout
    from makani_amd.losses import LossHandler
    from makani_amd.metric import MetricsHandler
    from makani_amd.sfnonet import SphericalFourierNeuralOperatorNet
    from makani_amd.stepper import SingleStepWrapper
    params = make_params(steps, [HELD])
    torch.manual_seed(0)
    wrap = SingleStepWrapper(params, lambda: SphericalFourierNeuralOperatorNet(**bench.CONFIG)).to(dev)
    wrap.eval()
    pp = wrap.preprocessor
    loss = LossHandler(params).to(dev)
    loss.eval()
    g = torch.Generator(device=dev).manual_seed(7)
    clim = 0.5 * torch.randn(C, H, W, device=dev, generator=g)
    means, stds = torch.rand(C, generator=torch.Generator().manual_seed(1)), 1.0 + torch.rand(C, generator=torch.Generator().manual_seed(2))
    means_d, stds_d = means.to(dev).view(1, C, 1, 1), stds.to(dev).view(1, C, 1, 1)
    oc = list(range(C))
    for B in (1, 2):
        inp = torch.randn(B, C, H, W, device=dev, generator=g)
        tar = torch.randn(B, steps, C, H, W, device=dev, generator=g)
        handlers = [MetricsHandler(params, torch.ones(C), clim, dev) for _ in range(2)]
        for h in handlers:
            h.initialize_buffers()
        ro = Rollout(params, wrap, metrics=handlers[0], loss=loss)
        space = torch.zeros(C, H, W, device=dev)
        over_time = torch.zeros(steps, C, device=dev)

        def through_rollout():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return ro.run(inp, tar, output_channels=oc, output_stats=(means, stds))

        def by_hand():
            out = []
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                inpt = inp
                for idt in range(steps):
                    targ = tar[:, idt]
                    pred = wrap(inpt).float()
                    pred[:, HELD] = inpt[:, HELD]
                    lval = loss(pred, targ, inpt)
                    handlers[1].update(pred, targ, lval, idt)
                    sqdif = (pred - targ) ** 2
                    over_time[idt] += torch.mean(sqdif, dim=(-1, -2)).sum(0)
                    for b in range(B):
                        space.add_(sqdif[b])
                    out.append((pred[:, oc] * stds_d + means_d).to("cpu"))
                    inpt = pp.append_history(inpt, pred, idt)
            return torch.stack(out)

        hip = with_knob("MK_ROLLOUT", "hip", through_rollout)
        err = rel(hip(), by_hand())
        assert err < 1e-5, err
        t_hip, t_hand = timed([hip, by_hand], args.window, args.rounds)
        r = dict(row=f"{steps}-step SFNO rollout", B=B, yn="bf16 autocast", hip_ms=round(t_hip * 1e3, 3), torch_ms=round(t_hand * 1e3, 3),
                 ratio=round(t_hand / t_hip, 3), err=err)
        rows.append(r)
        print(f"{r['row']:>28} B={B} {r['yn']:>14} {r['hip_ms']:>10.3f} {r['torch_ms']:>10.3f} {r['ratio']:>9.2f}", flush=True)
        del inp, tar, handlers, ro, space
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--part", default="tail,kernel,rollout", help="comma-separated groups of rows to run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rollout_bench: no GPU found")
    parts = set(args.part.split(","))
    assert parts <= {"tail", "kernel", "rollout"}, args.part
    from makani_amd import ops
    dev = torch.device("cuda:0")
    rows, kernels = [], []
    print(f"{'row':>28} {'B':>3} {'model output':>14} {'hip ms':>10} {'torch ms':>10} {'torch/hip':>9}")
    for B in (1, 2):
        for dtype, dname in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            if not parts & {"tail", "kernel"}:
                continue
            t = tail_inputs(dev, B, dtype)
            for name, kw in variants(t, dev):
                call = lambda: ops.rollout_tail(t["yn"], **kw)
                hip, tor = with_knob("MK_ROLLOUT", "hip", call), with_knob("MK_ROLLOUT", "torch", call)
                t["err"].zero_()
                a = hip()
                t["err"].zero_()
                b = tor()
                assert torch.equal(a[0], b[0]) and rel(a[1], b[1]) < 1e-6, (name, B, dname)
                del a, b
                if "tail" in parts:
                    t_hip, t_torch = timed([hip, tor], args.window, args.rounds)
                    r = dict(row=name, B=B, yn=dname, hip_ms=round(t_hip * 1e3, 4), torch_ms=round(t_torch * 1e3, 4),
                             ratio=round(t_torch / t_hip, 3))
                    rows.append(r)
                    print(f"{name:>28} {B:>3} {dname:>14} {r['hip_ms']:>10.3f} {r['torch_ms']:>10.3f} {r['ratio']:>9.2f}", flush=True)
                if "kernel" in parts:
                    for _ in range(2):
                        hip()
                    sec = window(hip, 10)
                    by = algorithmic_bytes(B, dtype, kw)
                    k = dict(kernel=name, B=B, yn=dname, ms=round(sec * 1e3, 4), bytes=by, TBs=round(by / sec / 1e12, 2))
                    kernels.append(k)
                    print(f"{'kernel: ' + name:>28} {B:>3} {dname:>14} {k['ms']:>10.3f} ms {k['TBs']:>6.2f} TB/s (algorithmic)", flush=True)
            del t
            torch.cuda.empty_cache()
    if "rollout" in parts:
        rollout_rows(dev, args.steps, args, rows)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="rollout_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r["ratio"] < 1.0]
    print(f"rollout_bench: done, {len(losing)} of {len(rows)} rows slower than the torch path")
    for r in losing:
        print(f"  slower: {r['row']} B={r['B']} {r['yn']} ({r['ratio']:.2f})")


if __name__ == "__main__":
    main()
