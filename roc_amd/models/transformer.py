"""Graph transformer: scaled dot-product attention over the in-neighbourhood
(PyG's TransformerConv; Shi et al. 2021, UniMP).

Per layer (H heads, concatenated; the last layer has 1 head):
  h = dropout(x);  q = h·Wq;  [K | V] = h·Wkv;  r = h·Wskip
  s(u→v) = <q_v, K_u> / sqrt(dh) per head;  alpha = softmax over v's in-edges
  y[v] = Σ_u alpha(u→v) · V_u + r[v]
Hidden layers close with ReLU, or with the fused LayerNorm + ReLU under
norm="layer" (models/norm.py).

K and V come out of one projection GEMM as one [n, 2*out] matrix and ride
one halo exchange; scores, softmax and the weighted sum of all heads are
one fused kernel per direction (ops.functional.graph_attention), so no
per-edge tensor exists. The reference has no attention model.

At world_size > 1 the shard must be in "halo" comm mode, as for GAT:
attention needs per-edge source rows (ROC_COMM_MODE=halo forces it).
"""
from __future__ import annotations

import torch

from ..ops import functional as F
from ..ops.reference import glorot_uniform
from ..parallel.halo import halo_exchange
from .norm import make_norm_params, hidden_act, norm_parameters


class GraphTransformer(torch.nn.Module):
    def __init__(self, dims, dropout: float = 0.5, seed: int = 1,
                 heads: int = 4, norm: str = "none"):
        super().__init__()
        self.norm = norm
        self.dims = list(dims)
        self.p = float(dropout)
        self.wq = torch.nn.ParameterList()
        self.wkv = torch.nn.ParameterList()
        self.wskip = torch.nn.ParameterList()
        self.heads = []
        for i in range(len(dims) - 1):
            h = heads if i < len(dims) - 2 else 1  # last layer: 1 head
            assert dims[i + 1] % h == 0, \
                f"layer {i}: out dim {dims[i + 1]} not divisible by {h} heads"
            self.heads.append(h)
            shape = (dims[i], dims[i + 1])
            self.wq.append(torch.nn.Parameter(
                glorot_uniform(shape, seed=seed + 4 * i)))
            # K and V halves drawn separately: fan-out is not doubled
            self.wkv.append(torch.nn.Parameter(torch.cat(
                [glorot_uniform(shape, seed=seed + 4 * i + 1),
                 glorot_uniform(shape, seed=seed + 4 * i + 2)], dim=1)))
            self.wskip.append(torch.nn.Parameter(
                glorot_uniform(shape, seed=seed + 4 * i + 3)))
        self.norm_gamma, self.norm_beta = make_norm_params(norm, dims)

    norm_parameters = norm_parameters

    recompute = False  # see GCN.recompute

    def forward(self, x, shard, group=None):
        if shard.world_size > 1:
            assert shard.comm_mode == "halo", (
                "GraphTransformer needs a halo-mode shard at world_size>1 "
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
        q = F.linear(h, self.wq[i])                 # [n_local, out]
        kv = F.linear(h, self.wkv[i])               # [n_local, 2*out]
        r = F.linear(h, self.wskip[i])
        kv_ext = halo_exchange(kv, shard, group)    # [n_ext, 2*out]
        y = F.add(F.graph_attention(q, kv_ext, shard, self.heads[i]), r)
        if i < len(self.wq) - 1:
            y = hidden_act(self, i, y)
        return y
