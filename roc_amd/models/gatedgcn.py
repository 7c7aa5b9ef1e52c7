"""GatedGCN: the residual gated graph ConvNet (Bresson & Laurent 2017; PyG's
ResGatedGraphConv, the GatedGCN of "Benchmarking GNNs" without edge
features, which the datasets here do not have).

Per layer:
  h = dropout(x);  [K | V] = h·Wkv;  q = h·Wq;  s = h·Ws
  eta(u→v) = sigmoid(q[v] + K[u])                    one gate per COLUMN
  y[v] = s[v] + Σ_u eta(u→v) ⊙ V[u]   (/ (Σ_u eta(u→v) + eps) if normalize)
Hidden layers close with ReLU, or with the fused norm + ReLU of
models/norm.py (norm="layer" or "sync_batch").

Every edge carries a vector of gates that depends on both of its end
points, so no per-edge scalar and no source-only weight can express it; the
fused kernels (ops.functional.gated_aggregate) gather [K | V] of each
neighbour once and keep the gates in registers: no per-edge tensor. K and V
come out of one projection GEMM as one [n, 2*out] matrix and ride one halo
exchange. normalize=True (the default) divides by the gate sum: on graphs
with hundreds of edges a row the plain gated sum scales with the degree.

At world_size > 1 the shard must be in "halo" comm mode, as for GAT: the
gates need per-edge source rows (ROC_COMM_MODE=halo forces it). Only kv
rides the halo exchange.
"""
from __future__ import annotations

import torch

from ..ops import functional as F
from ..ops.reference import glorot_uniform
from ..parallel.halo import halo_exchange
from .norm import make_norm_params, hidden_act, norm_parameters


class GatedGCN(torch.nn.Module):
    def __init__(self, dims, dropout: float = 0.5, seed: int = 1,
                 normalize: bool = True, norm: str = "none",
                 eps: float = 1e-6):
        super().__init__()
        self.norm = norm
        self.dims = list(dims)
        self.p = float(dropout)
        self.normalize = bool(normalize)
        self.eps = float(eps)
        self.wq = torch.nn.ParameterList()
        self.wkv = torch.nn.ParameterList()
        self.wskip = torch.nn.ParameterList()
        for i in range(len(dims) - 1):
            shape = (dims[i], dims[i + 1])
            self.wq.append(torch.nn.Parameter(
                glorot_uniform(shape, seed=seed + 4 * i)))
            # K and V halves drawn separately: fan-out is not doubled
            self.wkv.append(torch.nn.Parameter(torch.cat(
                [glorot_uniform(shape, seed=seed + 4 * i + 1),
                 glorot_uniform(shape, seed=seed + 4 * i + 2)], dim=1)))
            self.wskip.append(torch.nn.Parameter(
                glorot_uniform(shape, seed=seed + 4 * i + 3)))
        self.norm_gamma, self.norm_beta = make_norm_params(norm, dims, self)

    norm_parameters = norm_parameters

    recompute = False  # see GCN.recompute

    def forward(self, x, shard, group=None):
        if shard.world_size > 1:
            assert shard.comm_mode == "halo", (
                "GatedGCN needs a halo-mode shard at world_size>1 "
                f"(got '{shard.comm_mode}'; set ROC_COMM_MODE=halo)")
        for i in range(len(self.wq)):
            if self.recompute and self.training:
                x = torch.utils.checkpoint.checkpoint(
                    self._layer, i, x, shard, group,
                    use_reentrant=False, preserve_rng_state=False)
            else:
                x = self._layer(i, x, shard, group)
        return x

    def _layer(self, i, x, shard, group):
        h = F.dropout(x, self.p, self.training, call_id=i)
        kv = F.linear(h, self.wkv[i])               # [n_local, 2*out]
        q = F.linear(h, self.wq[i])                 # [n_local, out]
        s = F.linear(h, self.wskip[i])              # the root term
        kv_ext = halo_exchange(kv, shard, group)    # [n_ext, 2*out]
        y = F.add(s, F.gated_aggregate(q, kv_ext, shard, self.normalize,
                                       self.eps))
        if i < len(self.wq) - 1:
            y = hidden_act(self, i, y, shard, group)
        return y
