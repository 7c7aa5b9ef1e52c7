"""GATv2: dynamic graph attention (Brody et al. 2022, PyG's GATv2Conv).

Per layer (H heads, concatenated; the last layer has 1 head):
  h = dropout(x);  xl = h·Wl;  xr = h·Wr
  s(u→v) = a_h · LeakyReLU(xl[u,h,:] + xr[v,h,:])
  alpha = softmax over v's in-edges;  y[v,h,:] = Σ_u alpha(u→v) · xl[u,h,:]
Hidden layers close with ReLU, or with the fused LayerNorm + ReLU under
norm="layer" (models/norm.py).

GAT's score is a source scalar plus a destination scalar, so it ranks the
neighbours the same for every destination; here the nonlinearity sits
between the sum and the dot with a, so the ranking depends on the
destination. The price is that the score needs the whole source row per
edge; the fused kernels (ops.functional.gatv2_attention) gather that row
once and use it for the score and as the value, for all heads in one
launch per direction, with no per-edge tensor. The attention vectors are
fp32 masters [heads, dh] that the kernels read as fp32, like the norm's
gamma and beta. The reference has no attention model.

At world_size > 1 the shard must be in "halo" comm mode, as for GAT:
attention needs per-edge source rows (ROC_COMM_MODE=halo forces it). Only
xl rides the halo exchange.
"""
from __future__ import annotations

import torch

from ..ops import functional as F
from ..ops.reference import glorot_uniform
from ..parallel.halo import halo_exchange
from .norm import make_norm_params, hidden_act, norm_parameters


class GATv2(torch.nn.Module):
    def __init__(self, dims, dropout: float = 0.5, seed: int = 1,
                 heads: int = 4, negative_slope: float = 0.2,
                 norm: str = "none"):
        super().__init__()
        self.norm = norm
        self.dims = list(dims)
        self.p = float(dropout)
        self.slope = float(negative_slope)
        self.wl = torch.nn.ParameterList()
        self.wr = torch.nn.ParameterList()
        self.att = torch.nn.ParameterList()
        self.heads = []
        for i in range(len(dims) - 1):
            h = heads if i < len(dims) - 2 else 1  # last layer: 1 head
            assert dims[i + 1] % h == 0, \
                f"layer {i}: out dim {dims[i + 1]} not divisible by {h} heads"
            self.heads.append(h)
            shape = (dims[i], dims[i + 1])
            self.wl.append(torch.nn.Parameter(
                glorot_uniform(shape, seed=seed + 3 * i)))
            self.wr.append(torch.nn.Parameter(
                glorot_uniform(shape, seed=seed + 3 * i + 1)))
            self.att.append(torch.nn.Parameter(
                glorot_uniform((h, dims[i + 1] // h), seed=seed + 3 * i + 2)))
        self.norm_gamma, self.norm_beta = make_norm_params(norm, dims)

    norm_parameters = norm_parameters

    recompute = False  # see GCN.recompute

    def forward(self, x, shard, group=None):
        if shard.world_size > 1:
            assert shard.comm_mode == "halo", (
                "GATv2 needs a halo-mode shard at world_size>1 "
                f"(got '{shard.comm_mode}'; set ROC_COMM_MODE=halo)")
        for i in range(len(self.wl)):
            if self.recompute and self.training:
                x = torch.utils.checkpoint.checkpoint(
                    self._layer, i, x, shard, group,
                    use_reentrant=False, preserve_rng_state=False)
            else:
                x = self._layer(i, x, shard, group)
        return x

    def _layer(self, i, x, shard, group):
        h = F.dropout(x, self.p, self.training, call_id=i)
        xl = F.linear(h, self.wl[i])                # [n_local, out]
        xr = F.linear(h, self.wr[i])                # [n_local, out]
        xl_ext = halo_exchange(xl, shard, group)    # [n_ext, out]
        y = F.gatv2_attention(xl_ext, xr, self.att[i], shard, self.heads[i],
                              self.slope)
        if i < len(self.wl) - 1:
            y = hidden_act(self, i, y)
        return y
