"""Principal Neighbourhood Aggregation (Corso et al. 2020), single tower.

Layer i maps dims[i] -> dims[i+1]:

m  = h·W_msg                                  message transform
S  = [mean | std | max | min]_{u in N(v)} m_u one fused gather pass
hn = S·W_id + amp_v·(S·W_amp) + att_v·(S·W_att)
h' = act( h·W_self + hn )

The four aggregators come out of one gather of each neighbour row
(ops.functional.scatter_gather_stats), which runs at the OUTPUT width.
The three degree scalers — identity, amplification amp = log(d+1)/delta
and attenuation att = delta/log(d+1) — ride the GEMM's row_scale epilogue,
so the paper's [n, 12·d] concat is never materialised: its post-transform
is the sum of three [4·d, d] GEMMs.

delta is the mean of log(d+1) over all nodes of the WHOLE graph
(`pna_delta`), computed before sharding so that every rank holds the same
value; it is a buffer, not a parameter. d is the in-degree the shard
carries (`deg_local`, never below 1), or a block's sampled degree on the
mini-batch path.

norm="layer" replaces the hidden layers' relu with a fused per-node
LayerNorm + ReLU; see models/norm.py.
"""
from __future__ import annotations

import math

import torch

from ..ops import functional as F
from ..ops.reference import glorot_uniform
from ..parallel.aggregate import aggregate
from .norm import make_norm_params, hidden_act, norm_parameters


def pna_delta(g) -> float:
    """Mean of log(d+1) over every node of the whole graph g (a CSRGraph),
    d the in-degree clamped to 1 as the shards carry it."""
    deg = (g.rowptr[1:] - g.rowptr[:-1]).clamp(min=1).to(torch.float64)
    return float(torch.log(deg + 1.0).mean())


class PNA(torch.nn.Module):
    def __init__(self, dims, dropout: float = 0.5, seed: int = 1,
                 delta: float = None, norm: str = "none"):
        super().__init__()
        if delta is None or not (delta > 0 and math.isfinite(delta)):
            raise ValueError(
                f"PNA needs delta = pna_delta(graph) > 0, got {delta!r}")
        self.norm = norm
        self.dims = list(dims)
        self.p = float(dropout)
        self.register_buffer("delta", torch.tensor(float(delta)))
        # the float the forward uses (no device read on the hot path); a
        # loaded state_dict brings its own delta, so follow the buffer
        self._delta = float(delta)
        self.register_load_state_dict_post_hook(PNA._follow_delta)
        self.w_msg = torch.nn.ParameterList()
        self.w_self = torch.nn.ParameterList()
        self.w_id = torch.nn.ParameterList()
        self.w_amp = torch.nn.ParameterList()
        self.w_att = torch.nn.ParameterList()
        for i in range(len(dims) - 1):
            din, dout = dims[i], dims[i + 1]
            shapes = ((self.w_msg, (din, dout)), (self.w_self, (din, dout)),
                      (self.w_id, (4 * dout, dout)),
                      (self.w_amp, (4 * dout, dout)),
                      (self.w_att, (4 * dout, dout)))
            for j, (plist, shape) in enumerate(shapes):
                plist.append(torch.nn.Parameter(
                    glorot_uniform(shape, seed=seed + 5 * i + j)))
        self.norm_gamma, self.norm_beta = make_norm_params(norm, dims)

    norm_parameters = norm_parameters

    @staticmethod
    def _follow_delta(module, _incompatible_keys):
        module._delta = float(module.delta)

    recompute = False  # see GCN.recompute

    def scalers(self, deg):
        """(amp, att) fp32 [n] from the fp32 degrees (>= 1)."""
        lg = torch.log(deg.to(torch.float32) + 1.0)
        return (lg / self._delta).contiguous(), (self._delta / lg).contiguous()

    def forward(self, x, shard, group=None):
        amp, att = self.scalers(shard.deg_local)
        for i in range(len(self.w_self)):
            if self.recompute and self.training:
                x = torch.utils.checkpoint.checkpoint(
                    self._layer, i, x, shard, group, amp, att,
                    use_reentrant=False, preserve_rng_state=False)
            else:
                x = self._layer(i, x, shard, group, amp, att)
        return x

    def _post(self, i, h_dst, s, amp, att):
        """act( h·W_self + the three scaled transforms of the statistics )"""
        hn = F.add(F.linear(s, self.w_id[i]),
                   F.linear(s, self.w_amp[i], row_scale=amp))
        hn = F.add(hn, F.linear(s, self.w_att[i], row_scale=att))
        h = F.add(F.linear(h_dst, self.w_self[i]), hn)
        if i < len(self.w_self) - 1:
            h = hidden_act(self, i, h)
        return h

    def _layer(self, i, x, shard, group, amp, att):
        h = F.dropout(x, self.p, self.training, call_id=i)
        m = F.linear(h, self.w_msg[i])
        s = aggregate(m, shard, group=group, reduce="stats")
        return self._post(i, h, s, amp, att)

    def forward_blocks(self, x, blocks):
        """Mini-batch forward over sampled MFG blocks (roc_amd.sampling):
        layer i aggregates over blocks[i] and scales by its sampled
        degree; x holds the input features for blocks[0].src_ids rows.
        Returns [batch, dims[-1]]."""
        assert len(blocks) == len(self.w_self), (len(blocks), self.dims)
        for i in range(len(self.w_self)):
            blk = blocks[i]
            amp, att = self.scalers(1.0 / blk.inv_deg)
            h = F.dropout(x, self.p, self.training, call_id=i)
            m = F.linear(h, self.w_msg[i])
            s = F.scatter_gather_stats(m, blk)
            x = self._post(i, h[:blk.n_dst].contiguous(), s, amp, att)
        return x
