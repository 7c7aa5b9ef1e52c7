"""Training engine: per-rank epoch loop, gradient all-reduce, metrics.

The reference's train verbs (`Model::{init,forward,backward,update,
zero_gradients,train_mode,infer_mode}`, `gnn.h:162-203`) map to:
  Trainer.train_epoch  = zero_gradients + forward + backward + update
  Trainer.evaluate     = infer_mode + forward (metrics)
Weight-gradient reduction is a single fused RCCL all-reduce over a flat
bucket (the reference instead gathers grad replicas to ONE GPU and sums
serially, `optimizer_kernel.cu:88-94`).
"""
from __future__ import annotations

import copy
import time

import torch
import torch.distributed as dist

from .graph import MASK_TRAIN
from .ops import functional as F
from .optim import AdamOptimizer
from .parallel.partition import GraphShard


class Trainer:
    def __init__(self, model, shard: GraphShard, feats: torch.Tensor,
                 labels: torch.Tensor, mask: torch.Tensor,
                 optimizer: AdamOptimizer, device="cpu",
                 compute_dtype: torch.dtype = torch.float32,
                 grad_scale: float = 1.0, group=None, seed: int = 1,
                 num_classes=None, local_slices: bool = False,
                 gather_dtype=None):
        # local_slices=True: feats/labels/mask are ALREADY this rank's
        # [lo, hi) rows (windowed dataset loading)
        # gather_dtype="fp8": the sum aggregations gather e4m3 rows
        # (ops.functional.scatter_gather). The halo and allgather exchanges
        # stay bf16, so it is a single-process mode.
        if gather_dtype not in (None, "bf16", "fp8"):
            raise ValueError(f"gather_dtype must be 'bf16' or 'fp8', got "
                             f"{gather_dtype!r}")
        if gather_dtype == "fp8" and shard.world_size > 1:
            raise ValueError("gather_dtype='fp8' needs world size 1: the "
                             "halo and allgather paths gather bf16 rows")
        self.gather_dtype = gather_dtype
        self.model = model.to(device)
        self.device = torch.device(device)
        self.dtype = compute_dtype
        self.group = group
        self.grad_scale = grad_scale
        if local_slices:
            lo, hi = 0, shard.n_local
        else:
            lo, hi = shard.lo, shard.hi
        self.x = feats[lo:hi].to(device=device, dtype=compute_dtype).contiguous()
        self.labels = labels[lo:hi].to(device=device).contiguous()
        self.mask = mask[lo:hi].to(device=device, dtype=torch.int32).contiguous()
        self.shard = self._place_shard(shard, mask[lo:hi], device)
        self.optimizer = optimizer
        optimizer.setup_flat_grads()  # single-buffer grads (one all-reduce)
        self.num_classes = num_classes  # true classes if logits are padded
        self.clip_norm = 0.0  # >0: global grad-norm clip (branchless)
        self.epoch = 0
        F.set_dropout_seed(seed + shard.rank * 7919)
        self.tracer = None  # set via enable_tracing()

    def _place_shard(self, shard, mask, device):
        """The shard on the device, with the transpose plan of this
        trainer's loss rows: _forward_loss feeds the model's output to
        softmax_cross_entropy with this mask, whose gradient is zero on
        every row that is not a training row, for as long as the mask
        stays (models pass loss_rows_only=True on their last aggregation)."""
        shard = copy.copy(shard)  # the caller's shard keeps its plans
        shard.install_loss_rows(mask == MASK_TRAIN)
        shard = shard.to(device)
        shard.gather_dtype = self.gather_dtype
        return shard

    def enable_tracing(self):
        from .utils.trace import Tracer
        self.tracer = Tracer(device=str(self.device))
        return self.tracer

    def enable_offload(self, min_bytes: int = 1 << 22):
        """Host-DRAM activation offload (capacity tier, config #5)."""
        from .memory import ActivationOffload
        self.offload = ActivationOffload(min_bytes=min_bytes)
        return self.offload

    # -- hipGraph capture of the whole training epoch -----------------------
    # Launch-bound epochs (small shards / many GPUs) replay one hipGraph
    # instead of ~40 Python-driven launches. Epoch-varying state lives on
    # DEVICE: an int64 step counter bumped inside the graph drives the
    # Philox dropout offsets and the Adam bias-corrected/decayed step size.
    def enable_graph_capture(self, warmup_epochs: int = 2):
        assert self.device.type == "cuda", "graph capture needs a GPU"
        import os
        if self.shard.world_size > 1 and any(
                os.environ.get(v) == "1"
                for v in ("TORCH_NCCL_BLOCKING_WAIT", "NCCL_BLOCKING_WAIT")):
            # a blocking-wait collective inside a capture spins forever
            # (capture records, nothing executes — measured, r2c5);
            # refuse capture instead of hanging the job
            import sys
            print("[roc_amd] NCCL blocking-wait is on; hipGraph capture "
                  "of collectives would hang — staying eager",
                  file=sys.stderr, flush=True)
            return
        self._step_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        F.set_dropout_counter(self._step_dev)
        self.optimizer.set_device_step(self._step_dev)
        self._graph = None
        self._graph_warmup = warmup_epochs
        self._graph_metrics = None
        self.use_graph = True

    use_graph = False

    def _epoch_body(self):
        self._step_dev += 1
        F.reset_dropout_offset()
        self.optimizer.zero_grad()
        loss, metrics = self._forward_loss()
        if self.offload is not None:
            self.offload.prefetch()
        loss.backward()
        F.dw_flush()  # join side-stream dW GEMMs before grad consumers
        self._allreduce_grads()
        self.optimizer.step()
        return metrics

    def _graph_epoch(self):
        # (optimizer.step() inside _epoch_body increments host t itself;
        #  a replay executes no Python, so replays bump it explicitly)
        if self._graph is not None:
            self._graph.replay()
            self.optimizer.t += 1
            return self._graph_metrics
        if self._graph_warmup > 0:
            # warmup eagerly on a side stream (torch capture protocol)
            self._graph_warmup -= 1
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                metrics = self._epoch_body()
            torch.cuda.current_stream().wait_stream(s)
            return metrics
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._graph_metrics = self._epoch_body()
            self.optimizer.t -= 1  # capture recorded, did not execute
            self._graph = g
        except Exception as e:  # pragma: no cover - capture unsupported
            torch.cuda.synchronize()
            import sys
            print(f"[roc_amd] hipGraph capture failed ({e!r}); "
                  "falling back to eager", file=sys.stderr, flush=True)
            self.use_graph = False
            return self._epoch_body()
        self._graph.replay()
        self.optimizer.t += 1
        return self._graph_metrics

    # -- gradient all-reduce (flat buffer; weights are small) ---------------
    def _allreduce_grads(self):
        if self.shard.world_size > 1 and dist.is_initialized():
            dist.all_reduce(self.optimizer._flat_grad, group=self.group)
        if self.clip_norm > 0:
            # branchless global-norm clip on the flat buffer: scale by
            # clip/max(norm, clip) — 1.0 when under the bound. No host
            # readback or data-dependent branch, so it works inside
            # hipGraph capture (post-all-reduce: every rank scales the
            # same summed gradient identically).
            g = self.optimizer._flat_grad
            norm = torch.linalg.vector_norm(g)
            g.mul_(self.clip_norm / torch.clamp(norm, min=self.clip_norm))

    offload = None  # set via enable_offload()

    def _forward_loss(self):
        if self.offload is not None:
            with self.offload:
                logits = self.model(self.x, self.shard, self.group)
                return F.softmax_cross_entropy(
                    logits, self.labels, self.mask, self.grad_scale,
                    self.num_classes)
        logits = self.model(self.x, self.shard, self.group)
        return F.softmax_cross_entropy(
            logits, self.labels, self.mask, self.grad_scale,
            self.num_classes)

    def train_epoch(self):
        self.model.train()
        if (self.use_graph and self.device.type == "cuda"
                and self.tracer is None and self.offload is None
                and not getattr(self.model, "recompute", False)):
            metrics = self._graph_epoch()
            self.epoch += 1
            return metrics
        F.next_dropout_epoch()
        if self.tracer is None:
            self.optimizer.zero_grad()
            loss, metrics = self._forward_loss()
            if self.offload is not None:
                self.offload.prefetch()
            loss.backward()
            F.dw_flush()
            self._allreduce_grads()
            self.optimizer.step()
        else:
            tr = self.tracer
            with tr.span("zero_grad"):
                self.optimizer.zero_grad()
            with tr.span("forward"):
                loss, metrics = self._forward_loss()
            with tr.span("backward"):
                if self.offload is not None:
                    self.offload.prefetch()
                loss.backward()
                F.dw_flush()
            with tr.span("grad_allreduce"):
                self._allreduce_grads()
            with tr.span("adam"):
                self.optimizer.step()
            tr.next_epoch()
        self.epoch += 1
        return metrics

    @torch.no_grad()
    def evaluate(self) -> dict:
        self.model.eval()
        logits = self.model(self.x, self.shard, self.group)
        _, metrics = F.softmax_cross_entropy(
            logits, self.labels, self.mask, self.grad_scale,
            self.num_classes)
        if self.shard.world_size > 1 and dist.is_initialized():
            dist.all_reduce(metrics, group=self.group)
        return F.decode_metrics(metrics)

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    # -- reference train-verb API (gnn.h:162-203 parity) --------------------
    # train_epoch() is the packaged loop; these verbs expose the same
    # steps individually, in the reference's vocabulary.
    def train_mode(self):
        self.model.train()

    def infer_mode(self):
        self.model.eval()

    def zero_gradients(self):
        # once-per-epoch in the reference loop (`gnn.cc:103`) — the right
        # place to advance the dropout epoch base, matching train_epoch
        F.next_dropout_epoch()
        self.optimizer.zero_grad()

    def forward(self):
        self._last_loss, self._last_metrics = self._forward_loss()
        return self._last_metrics

    def backward(self):
        if self.offload is not None:
            self.offload.prefetch()
        self._last_loss.backward()
        F.dw_flush()

    def update(self):
        self._allreduce_grads()
        self.optimizer.step()

    # -- cost-model repartitioning (the MLSys'20 Roc idea; the reference
    #    code only has the static edge-balanced split) --------------------
    def measure_and_rebalance(self, feats=None, labels=None, mask=None,
                              probe_epochs=3):
        """Measure this rank's epoch time, gather every rank's (time,
        halo-rows) over the gloo control plane, fit the comm-aware cost
        model t ≈ a*edges + b*halo, re-split the vertex ranges so
        predicted times equalize, and rebuild the shard in place.

        Two data modes: full (attach_full_graph + full feats/labels/mask
        on every rank) or windowed (attach_windowed_dataset — each rank
        re-reads only its new window from the dataset files).
        Returns the new bounds."""
        from .parallel.comm import cpu_group
        from .parallel.partition import (rebalance_bounds_comm, build_shard,
                                         build_shard_from_lux)
        t = self.timed_epochs(probe_epochs) / probe_epochs
        if self.shard.world_size == 1 or not dist.is_initialized():
            return self.shard.bounds
        ws = self.shard.world_size
        g = cpu_group(self.group)
        stats = torch.zeros(ws, 2, dtype=torch.float64)
        stats[self.shard.rank, 0] = t
        stats[self.shard.rank, 1] = float(self.shard.n_halo)
        dist.all_reduce(stats, group=g)
        if not hasattr(self, "_rebal_samples"):
            self._rebal_samples = []
        new_bounds = rebalance_bounds_comm(
            self._full_rowptr, self.shard.bounds, stats[:, 0].tolist(),
            stats[:, 1].tolist(), self._rebal_samples)
        if new_bounds == self.shard.bounds:
            return new_bounds
        if getattr(self, "_window_loader", None) is not None:
            new_shard = build_shard_from_lux(
                self._lux_path, self.shard.rank, ws, new_bounds,
                group=self.group)
            feats, labels, mask = self._window_loader(
                new_shard.lo, new_shard.hi)
            self.load_shard(new_shard, feats, labels, mask,
                            local_slices=True)
        else:
            new_shard = build_shard(self._full_graph, self.shard.rank,
                                    ws, new_bounds,
                                    use_comm=dist.is_initialized(),
                                    group=self.group)
            self.load_shard(new_shard, feats, labels, mask)
        return new_bounds

    def attach_full_graph(self, g):
        """Keep a handle to the full CPU graph for repartitioning."""
        self._full_graph = g
        self._full_rowptr = g.rowptr

    def attach_windowed_dataset(self, lux_path: str, window_loader,
                                rowptr: torch.Tensor):
        """Repartitioning under windowed file loading: `window_loader(lo,
        hi)` returns this rank's (feats, labels, mask) rows; `rowptr` is
        the full-graph row pointer (cheap: 8 B/vertex, already read by
        load_lux_meta)."""
        self._lux_path = lux_path
        self._window_loader = window_loader
        self._full_rowptr = rowptr

    def load_shard(self, shard, feats, labels, mask, local_slices=False):
        device, dt = self.device, self.dtype
        lo, hi = (0, shard.n_local) if local_slices else (shard.lo, shard.hi)
        self.shard = self._place_shard(shard, mask[lo:hi], device)
        self.x = feats[lo:hi].to(device=device, dtype=dt).contiguous()
        self.labels = labels[lo:hi].to(device=device).contiguous()
        self.mask = mask[lo:hi].to(device=device,
                                   dtype=torch.int32).contiguous()

    def timed_epochs(self, n: int) -> float:
        """Run n training epochs, return wall seconds (caller barriers)."""
        self.sync()
        t0 = time.perf_counter()
        for _ in range(n):
            self.train_epoch()
        self.sync()
        return time.perf_counter() - t0
