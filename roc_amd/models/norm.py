"""Hidden-layer normalization shared by GCN, GraphSAGE and GIN.

norm="layer" closes every hidden layer (not the last one) with a per-node
LayerNorm + ReLU in one fused kernel instead of the plain ReLU. gamma
starts at ones and beta at zeros, both fp32 masters; no RNG is drawn, so
the linear weights of a seed are the same with and without the norm.
With norm="none" the lists below are empty: no parameter, no
state_dict key.
"""
from __future__ import annotations

import torch

from ..ops import functional as F

NORMS = ("none", "layer")


def make_norm_params(norm: str, dims):
    """(gammas, betas): one fp32 [dims[i+1]] pair per hidden layer."""
    if norm not in NORMS:
        raise ValueError(f"norm must be 'none' or 'layer', got {norm!r}")
    gammas, betas = torch.nn.ParameterList(), torch.nn.ParameterList()
    if norm == "layer":
        for i in range(len(dims) - 2):
            gammas.append(torch.nn.Parameter(torch.ones(dims[i + 1])))
            betas.append(torch.nn.Parameter(torch.zeros(dims[i + 1])))
    return gammas, betas


def hidden_act(model, i: int, h):
    """The closing activation of hidden layer i of `model`."""
    if model.norm == "layer":
        return F.layer_norm(h, model.norm_gamma[i], model.norm_beta[i],
                            activation="relu")
    return F.relu(h)


def norm_parameters(model):
    """The gammas and betas (parameters that take no weight decay)."""
    return list(model.norm_gamma) + list(model.norm_beta)
