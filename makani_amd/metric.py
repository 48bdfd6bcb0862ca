"""``MetricsHandler`` of the trainer's validation loop (``makani/utils/metric.py:27-306``, called by
``Trainer.validate_one_epoch``, trainer.py:799-875): per autoregressive step it accumulates the ACC and RMSE curves of
every output channel, the validation loss and the geometric L1; ``finalize`` reduces over the data-parallel ranks and
assembles the logs.  Same constructor, methods, buffers (fp32), log keys and arithmetic as the reference.

Deliberate differences:

- ``update`` does not synchronise with the host: one ``ops.geo_metric_sums`` pass gives the five latitude-weighted
  integrals per (sample, channel) that every metric is made of, and the epilogue on ``[B, C]`` stays on the device, so
  a rollout of updates can be captured into one graph.
- Spatial model parallelism reduces partial sums instead of gathering the fields: each rank slices the climatology and
  the latitude weights to its own ``h`` / ``w`` shard once, at construction, computes its sums and all-reduces the
  ``[B, C, 5]`` float64 sums over the ``"spatial"`` group; the ratios and roots are formed after that reduction.
  ``_gather_input`` stays for the trainer's visualisation.
- ``"rollouts"`` is a ``wandb.Table`` when ``wandb`` imports, else ``{"columns": [...], "data": [...]}``.
- No ``torch.compile``.
- Channel (matmul) parallelism raises ``NotImplementedError`` (the reference's branch uses an undefined ``valid_l1``,
  metric.py:225).
- ``finalize``'s barrier passes ``device_ids`` only on the nccl backend, so gloo works.
"""
import torch
import torch.distributed as dist

from . import comm, ops
from .distributed import all_reduce_spatial, compute_split_shapes, shard_span
from .mappings import gather_from_parallel_region
from .metrics import GeometricACC, GeometricL1, GeometricRMSE, Quadrature

_DEFAULT_VARS = ["u10m", "t2m", "u500", "z500", "r500", "q500"]
_ROLLOUT_COLUMNS = ["metric type", "variable name", "time [h]", "value"]


def _rollouts_table(data, columns):
    try:
        import wandb
    except ImportError:
        return {"columns": list(columns), "data": data}
    return wandb.Table(data=data, columns=columns)


class MetricsHandler:
    """Buffers and arithmetic of the validation metrics (metric.py:27-306)."""

    def __init__(self, params, mult, clim, device, rmse_var_names=_DEFAULT_VARS, acc_vars_names=_DEFAULT_VARS,
                 acc_auc_var_names=_DEFAULT_VARS):
        self.device = torch.device(device)
        self.log_to_screen = params.log_to_screen
        self.log_to_wandb = params.log_to_wandb
        self.channel_names = params.channel_names

        # effective time interval and steps per day
        self.dtxdh = params.dt * params.dhours
        self.dd = 24 // self.dtxdh

        # the variables actually present, and their channel indices
        self.rmse_vars = {n: self.channel_names.index(n) for n in rmse_var_names if n in self.channel_names}
        self.acc_vars = {n: self.channel_names.index(n) for n in acc_vars_names if n in self.channel_names}
        self.acc_auc_vars = {n: self.channel_names.index(n) for n in acc_auc_var_names if n in self.channel_names}

        self.split_data_channels = params.split_data_channels
        if self.split_data_channels and comm.get_size("matmul") > 1:
            raise NotImplementedError("MetricsHandler: channel (matmul) parallelism is not supported")

        self.mult = mult.to(self.device)
        self.valid_autoreg_steps = params.valid_autoreg_steps
        self.simpquad = Quadrature(self.valid_autoreg_steps, 1.0 / float(self.valid_autoreg_steps + 1), self.device)

        self.N_out_channels = params.N_out_channels
        self.out_channels_local = params.N_out_channels

        self.img_shape = (params.img_shape_x, params.img_shape_y)
        self.crop_shape = (params.img_crop_shape_x, params.img_crop_shape_y)
        self.crop_offset = (params.img_crop_offset_x, params.img_crop_offset_y)
        quadrature_rule_type = "legendre-gauss" if params.model_grid_type == "legendre_gauss" else "naive"

        # the reference's metric objects (same configuration); update() itself works from their shared weights
        common = dict(img_shape=self.img_shape, crop_shape=self.crop_shape, crop_offset=self.crop_offset, normalize=True)
        self.l1_handle = GeometricL1(quadrature_rule_type, channel_reduction="mean", batch_reduction="sum", **common).to(self.device)
        self.rmse_handle = GeometricRMSE(quadrature_rule_type, channel_reduction="none", batch_reduction="none",
                                         **common).to(self.device)
        self.acc_handle = GeometricACC(quadrature_rule_type, channel_reduction="none", batch_reduction="sum",
                                       **common).to(self.device)
        self.acc_eps = self.acc_handle.eps

        # this rank's shard of the latitude weights and of the climatology ([C, H, W] over the crop)
        (h0, hs), (w0, ws) = shard_span(self.crop_shape[0], "h"), shard_span(self.crop_shape[1], "w")
        self.wrow = self.rmse_handle.quadrature.row_weights[h0:h0 + hs].float().contiguous()
        self.clim = clim.to(self.device, dtype=torch.float32)[..., h0:h0 + hs, w0:w0 + ws].contiguous()
        self.do_gather_input = comm.get_size("spatial") > 1
        if self.do_gather_input:
            self.gather_shapes_h = compute_split_shapes(self.crop_shape[0], comm.get_size("h"))
            self.gather_shapes_w = compute_split_shapes(self.crop_shape[1], comm.get_size("w"))

    def _gather_input(self, x):
        """gather the spatial shards of x over h, then w"""
        xh = gather_from_parallel_region(x, -2, self.gather_shapes_h, "h")
        return gather_from_parallel_region(xh, -1, self.gather_shapes_w, "w")

    def initialize_buffers(self):
        """buffers of the validation metrics, the ACC / RMSE curves and their host copies"""
        steps = self.valid_autoreg_steps + 1
        self.valid_buffer = torch.zeros((3), dtype=torch.float32, device=self.device)
        self.valid_loss = self.valid_buffer[0].view(-1)
        self.valid_l1 = self.valid_buffer[1].view(-1)
        self.valid_steps = self.valid_buffer[2].view(-1)

        self.acc_curve = torch.zeros((self.out_channels_local, steps), dtype=torch.float32, device=self.device)
        self.rmse_curve = torch.zeros((self.out_channels_local, steps), dtype=torch.float32, device=self.device)
        self.acc_counter = torch.zeros((steps), dtype=torch.float32, device=self.device)

        pin_memory = self.device.type == "cuda"
        self.valid_buffer_cpu = torch.zeros((3), dtype=torch.float32, device="cpu", pin_memory=pin_memory)
        self.acc_curve_cpu = torch.zeros((self.out_channels_local, steps), dtype=torch.float32, device="cpu", pin_memory=pin_memory)
        self.acc_auc_cpu = torch.zeros((self.out_channels_local), dtype=torch.float32, device="cpu", pin_memory=pin_memory)
        self.rmse_curve_cpu = torch.zeros((self.out_channels_local, steps), dtype=torch.float32, device="cpu", pin_memory=pin_memory)

    def zero_buffers(self):
        """set buffers to zero"""
        with torch.no_grad():
            self.valid_buffer.fill_(0)
            self.acc_curve.fill_(0)
            self.rmse_curve.fill_(0)
            self.acc_counter.fill_(0)

    def _global_sums(self, prediction, target):
        """[B, C, 5] float64 sums over the whole (cropped) field: this rank's shard, all-reduced over the spatial group."""
        return all_reduce_spatial(ops.geo_metric_sums(prediction, target, self.clim, self.wrow))

    def update(self, prediction, target, loss, idt):
        """accumulate one autoregressive step; no host synchronisation"""
        with torch.no_grad():
            s = self._global_sums(prediction, target)
            acc = s[..., 2] / (torch.sqrt(s[..., 3] * s[..., 4]) + self.acc_eps)        # GeometricACC, per (b, c)
            self.acc_curve[:, idt] += torch.sum(acc, dim=0).float()
            self.rmse_curve[:, idt] += self.mult * torch.sum(torch.sqrt(s[..., 1]), dim=0).float()
            self.acc_counter[idt] += 1
            if idt == 0:
                self.valid_steps += 1.0
                self.valid_loss += loss
                self.valid_l1 += torch.sum(torch.mean(s[..., 0], dim=1), dim=0).float()

    def finalize(self, final_inference=False):
        """reduce over the data-parallel ranks and assemble the logs"""
        if dist.is_initialized():
            if dist.get_backend() == "nccl":
                dist.barrier(device_ids=[self.device.index])
            else:
                dist.barrier()

        with torch.no_grad():
            valid_steps_local = int(self.valid_steps.item())

            if dist.is_initialized() and comm.get_size("data") > 1:
                grp = comm.get_group("data")
                dist.all_reduce(self.valid_buffer, op=dist.ReduceOp.SUM, group=grp)
                dist.all_reduce(self.acc_curve, op=dist.ReduceOp.SUM, group=grp)
                dist.all_reduce(self.rmse_curve, op=dist.ReduceOp.SUM, group=grp)
                dist.all_reduce(self.acc_counter, op=dist.ReduceOp.SUM, group=grp)

            self.valid_buffer[0:2] = self.valid_buffer[0:2] / self.valid_buffer[2]
            self.acc_curve /= self.acc_counter
            self.rmse_curve /= self.acc_counter
            acc_auc = self.simpquad(self.acc_curve, dim=1)

            self.valid_buffer_cpu.copy_(self.valid_buffer)
            self.acc_curve_cpu.copy_(self.acc_curve)
            self.rmse_curve_cpu.copy_(self.rmse_curve)
            self.acc_auc_cpu.copy_(acc_auc)

            valid_buffer_arr = self.valid_buffer_cpu.numpy()
            logs = {"base": {"validation steps": valid_steps_local, "validation loss": valid_buffer_arr[0],
                             "validation L1": valid_buffer_arr[1]}, "metrics": {}}

            valid_rmse_arr = self.rmse_curve_cpu[:, 0].numpy()
            for var_name, var_idx in self.rmse_vars.items():
                logs["metrics"]["validation " + var_name] = valid_rmse_arr[var_idx]

            acc_auc_arr = self.acc_auc_cpu.numpy()
            for var_name, var_idx in self.acc_auc_vars.items():
                logs["metrics"]["ACC AUC " + var_name] = acc_auc_arr[var_idx]

            table_data = []
            acc_curve_arr = self.acc_curve_cpu.numpy()
            for var_name, var_idx in self.acc_vars.items():
                for d in range(0, self.valid_autoreg_steps + 1):
                    table_data.append(["ACC", f"{var_name}", (d + 1) * self.dtxdh, acc_curve_arr[var_idx, d]])
            rmse_curve_arr = self.rmse_curve_cpu.numpy()
            for var_name, var_idx in self.rmse_vars.items():
                for d in range(0, self.valid_autoreg_steps + 1):
                    table_data.append(["RMSE", f"{var_name}", (d + 1) * self.dtxdh, rmse_curve_arr[var_idx, d]])
            logs["metrics"]["rollouts"] = _rollouts_table(table_data, _ROLLOUT_COLUMNS)

        self.logs = logs
        if final_inference:
            return logs, self.acc_curve, self.rmse_curve
        return logs
