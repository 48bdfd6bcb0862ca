"""MetricsHandler.update on the production field [B, 73, 721, 1440] (B = 1, 2; fp32 and bf16 predictions), one process:
the HIP path (ops.geo_metric_sums + the [B, C] epilogue) alternated with a restatement of the reference's formulation
in eager torch (makani/utils/metric.py:186-204 with functions.py:20-107, without torch.compile).  Each update is the
idt = 0 one (ACC, RMSE and L1).  Medians of device-event times; GB/s against the algorithmic bytes
B (bytes(p) + 4) HW C + 4 HW C (prediction, target, climatology read once).  The copy ceiling of this machine's HBM
for row-segment streams is 4.5-5.3 TB/s (profiles/r02_membench.txt).

    python tools/metrics_bench.py [--quick] [--iters N]

--quick: 3 updates of the HIP path alone at B = 1 fp32, so that a kernel trace (rocprofv3 --kernel-trace --stats) shows
what one update launches."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from makani_amd.metric import MetricsHandler  # noqa: E402

C, H, W = 73, 721, 1440


class EagerReference:
    """The reference handler's update in eager torch: gather-free, same buffers, same arithmetic."""

    def __init__(self, handler):
        self.q = handler.rmse_handle.quadrature.quad_weight          # [1, 1, H, W]
        self.clim = handler.clim.unsqueeze(0)
        self.mult = handler.mult
        self.acc_curve = torch.zeros_like(handler.acc_curve)
        self.rmse_curve = torch.zeros_like(handler.rmse_curve)
        self.acc_counter = torch.zeros_like(handler.acc_counter)
        self.valid_buffer = torch.zeros_like(handler.valid_buffer)
        self.eps = handler.acc_eps

    def quad(self, x):
        return torch.sum(x * self.q, dim=(-2, -1))

    def update(self, prediction, target, loss, idt):
        x, y = prediction - self.clim, target - self.clim
        acc = self.quad(x * y) / (torch.sqrt(self.quad(torch.square(x)) * self.quad(torch.square(y))) + self.eps)
        self.acc_curve[:, idt] += torch.sum(acc, dim=0)
        self.rmse_curve[:, idt] += self.mult * torch.sum(torch.sqrt(self.quad(torch.square(prediction - target))), dim=0)
        self.acc_counter[idt] += 1
        if idt == 0:
            self.valid_buffer[2] += 1.0
            self.valid_buffer[0] += loss
            self.valid_buffer[1] += torch.sum(torch.mean(self.quad(torch.abs(prediction - target)), dim=1), dim=0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    names = ["u10m", "t2m", "z500"] + [f"c{i}" for i in range(C - 3)]
    params = SimpleNamespace(log_to_screen=False, log_to_wandb=False, channel_names=names, dt=1, dhours=6,
                             split_data_channels=False, valid_autoreg_steps=2, N_out_channels=C, img_shape_x=H,
                             img_shape_y=W, img_crop_shape_x=H, img_crop_shape_y=W, img_crop_offset_x=0, img_crop_offset_y=0,
                             model_grid_type="equiangular")
    g = torch.Generator(device=dev).manual_seed(7)
    clim = torch.randn(C, H, W, device=dev, generator=g)
    cases = [(1, torch.float32)] if args.quick else [(1, torch.float32), (1, torch.bfloat16), (2, torch.float32),
                                                     (2, torch.bfloat16)]
    iters = 3 if args.quick else args.iters
    rows = []
    with torch.inference_mode():
        for B, dtype in cases:
            tar = clim + torch.randn(B, C, H, W, device=dev, generator=g)
            prd = (tar + 0.3 * torch.randn(B, C, H, W, device=dev, generator=g)).to(dtype)
            loss = torch.rand((), device=dev, generator=g)
            handler = MetricsHandler(params, torch.ones(C), clim, dev)
            handler.initialize_buffers()
            ref = EagerReference(handler)
            t_hip, t_ref = [], []
            if args.quick:
                for _ in range(iters):
                    t_hip.append(timed(lambda: handler.update(prd, tar, loss, 0)))
                t_ref = [float("nan")]
            else:
                for _ in range(2):                                        # warm-up
                    handler.update(prd, tar, loss, 0)
                    ref.update(prd, tar, loss, 0)
                for _ in range(iters):
                    t_hip.append(timed(lambda: handler.update(prd, tar, loss, 0)))
                    t_ref.append(timed(lambda: ref.update(prd, tar, loss, 0)))
            nbytes = B * (prd.element_size() + 4) * H * W * C + 4 * H * W * C
            mh, mr = statistics.median(t_hip), statistics.median(t_ref)
            row = dict(B=B, dtype=str(dtype).replace("torch.", ""), MB=round(nbytes / 1e6, 1), hip_ms=round(mh, 4),
                       eager_ms=round(mr, 4), hip_TBps=round(nbytes / mh / 1e9, 2), speedup=round(mr / mh, 1))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del tar, prd, handler, ref
            torch.cuda.empty_cache()
    return rows


if __name__ == "__main__":
    main()
