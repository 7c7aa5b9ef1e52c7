"""Hidden-layer normalization shared by GCN, GraphSAGE and GIN.

norm="layer" closes every hidden layer (not the last one) with a per-node
LayerNorm + ReLU in one fused kernel instead of the plain ReLU.
norm="sync_batch" closes it with BatchNorm + ReLU over the nodes of ALL
shards (ops.functional.batch_norm; the statistics are synchronised across
ranks, hence the name): batch statistics in training, the running
statistics in eval. gamma starts at ones and beta at zeros, both fp32
masters; no RNG is drawn, so the linear weights of a seed are the same with
and without the norm. With norm="none" the lists below are empty: no
parameter, no state_dict key.
"""
from __future__ import annotations

import torch

from ..ops import functional as F

NORMS = ("none", "layer", "sync_batch")


def make_norm_params(norm: str, dims, module=None):
    """(gammas, betas): one fp32 [dims[i+1]] pair per hidden layer. With
    norm="sync_batch" also registers on `module` the buffers
    norm_running_mean_<i> (zeros) and norm_running_var_<i> (ones): state
    that travels in state_dict and is no optimizer parameter."""
    if norm not in NORMS:
        raise ValueError(
            f"norm must be 'none', 'layer' or 'sync_batch', got {norm!r}")
    gammas, betas = torch.nn.ParameterList(), torch.nn.ParameterList()
    if norm != "none":
        for i in range(len(dims) - 2):
            gammas.append(torch.nn.Parameter(torch.ones(dims[i + 1])))
            betas.append(torch.nn.Parameter(torch.zeros(dims[i + 1])))
    if norm == "sync_batch":
        for i in range(len(dims) - 2):
            module.register_buffer(f"norm_running_mean_{i}",
                                   torch.zeros(dims[i + 1]))
            module.register_buffer(f"norm_running_var_{i}",
                                   torch.ones(dims[i + 1]))
    return gammas, betas


def running_stats(model, i: int):
    """(running_mean, running_var) of hidden layer i of a
    norm="sync_batch" model."""
    return (getattr(model, f"norm_running_mean_{i}"),
            getattr(model, f"norm_running_var_{i}"))


def hidden_act(model, i: int, h, shard=None, group=None):
    """The closing activation of hidden layer i of `model`. `shard` tells
    norm="sync_batch" how many ranks share the rows and how many rows there are
    in all; without it (a sampled block) the batch is h's own rows."""
    if model.norm == "layer":
        return F.layer_norm(h, model.norm_gamma[i], model.norm_beta[i],
                            activation="relu")
    if model.norm == "sync_batch":
        ws = shard.world_size if shard is not None else 1
        return F.batch_norm(h, model.norm_gamma[i], model.norm_beta[i],
                            *running_stats(model, i),
                            training=model.training, activation="relu",
                            group=group, world_size=ws,
                            n_total=shard.bounds[-1] if ws > 1 else None)
    return F.relu(h)


def norm_parameters(model):
    """The gammas and betas (parameters that take no weight decay)."""
    return list(model.norm_gamma) + list(model.norm_beta)
