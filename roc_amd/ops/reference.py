"""Plain-PyTorch reference implementations of every operator.

These are the numerics oracle for the HIP kernels (tests compare the
CDNA4 kernels against these in fp32) and the execution path for the
CPU-only Cora config. Semantics mirror the reference ops
(`/root/reference/*_kernel.cu`), cited per function.
"""
from __future__ import annotations

import torch

from ..graph import MASK_TRAIN, MASK_VAL, MASK_TEST


def spmm(x: torch.Tensor, rowptr: torch.Tensor, colidx: torch.Tensor,
         num_rows: int) -> torch.Tensor:
    """out[v] = sum_{u in N_in(v)} x[u]  (reference `scattergather_kernel.cu:20-76`).

    x may have more rows than num_rows (halo-extended input).
    """
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.long)
    dst = torch.repeat_interleave(
        torch.arange(num_rows, dtype=torch.long, device=x.device), deg
    )
    out = torch.zeros(num_rows, x.shape[1], dtype=x.dtype, device=x.device)
    out.index_add_(0, dst, x[colidx.to(torch.long)])
    return out


def spmm_weighted(x: torch.Tensor, rowptr: torch.Tensor,
                  colidx: torch.Tensor, edge_val: torch.Tensor,
                  num_rows: int) -> torch.Tensor:
    """out[v] = sum_{e in row v} edge_val[e] * x[col_e]  — the edge-tensor
    consumer op (the reference declares per-edge tensors,
    `gnn.cc:475-623` create_edge_tensor, but ships no op over them)."""
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.long)
    dst = torch.repeat_interleave(
        torch.arange(num_rows, dtype=torch.long, device=x.device), deg
    )
    out = torch.zeros(num_rows, x.shape[1], dtype=x.dtype, device=x.device)
    out.index_add_(0, dst,
                   x[colidx.to(torch.long)] * edge_val.unsqueeze(1).to(x.dtype))
    return out


def edge_dot(dy: torch.Tensor, x: torch.Tensor, rowptr: torch.Tensor,
             colidx: torch.Tensor) -> torch.Tensor:
    """dval[e] = <dy[row_e], x[col_e]> — gradient of spmm_weighted wrt
    the per-edge values (fp32 accumulate)."""
    num_rows = rowptr.numel() - 1
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.long)
    dst = torch.repeat_interleave(
        torch.arange(num_rows, dtype=torch.long, device=dy.device), deg
    )
    return (dy[dst].float() * x[colidx.to(torch.long)].float()).sum(dim=1)


def seg_max(x: torch.Tensor, rowptr: torch.Tensor, colidx: torch.Tensor,
            num_rows: int, reduce: str = "max"):
    """out[v, j] = max (or min) over the edges e of row v of x[colidx[e], j];
    arg[v, j] (int32) = the CSR edge index e of the winner. Among equal
    values the FIRST edge in CSR order wins; an empty row gives out = 0,
    arg = -1. The reference declares AGGR_MAX / AGGR_MIN (`gnn.h:75-79`)
    and implements neither. NaN inputs are out of contract.

    arg names an edge, not a source row, so that duplicate (u, v) edges
    route the gradient once. out is read back through arg, so it carries
    the winning input's own bits (low-precision x is compared in fp32)."""
    if reduce not in ("max", "min"):
        raise ValueError(f"reduce must be 'max' or 'min', got {reduce!r}")
    E, D = int(colidx.numel()), x.shape[1]
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.long)
    dst = torch.repeat_interleave(
        torch.arange(num_rows, dtype=torch.long, device=x.device), deg)
    wide = x.dtype in (torch.float32, torch.float64)
    vals = (x if wide else x.float())[colidx.to(torch.long)]  # [E, D]
    idx = dst.unsqueeze(1).expand(E, D)
    best = torch.zeros(num_rows, D, dtype=vals.dtype, device=x.device)
    best = best.scatter_reduce(0, idx, vals,
                               reduce="amax" if reduce == "max" else "amin",
                               include_self=False)
    eid = torch.arange(E, dtype=torch.long, device=x.device).unsqueeze(1)
    cand = torch.where(vals == best[dst], eid.expand(E, D),
                       torch.full((), E, dtype=torch.long, device=x.device))
    arg = torch.full((num_rows, D), E, dtype=torch.long, device=x.device)
    arg = arg.scatter_reduce(0, idx, cand, reduce="amin", include_self=True)
    empty = (deg == 0).unsqueeze(1)
    arg = arg.masked_fill(empty, 0)
    if E > 0:
        out = torch.gather(vals, 0, arg).masked_fill(empty, 0)
    else:
        out = torch.zeros(num_rows, D, dtype=vals.dtype, device=x.device)
    arg = arg.masked_fill(empty, -1).to(torch.int32)
    return out.to(x.dtype), arg


def seg_max_grad(dy: torch.Tensor, arg: torch.Tensor, rowptr: torch.Tensor,
                 colidx: torch.Tensor, num_src: int) -> torch.Tensor:
    """Gradient of seg_max wrt x: dy[v, j] goes, whole, to source row
    colidx[arg[v, j]] (first-edge routing — torch's own amax backward
    splits ties evenly, so it is not the oracle here). rowptr is unused:
    arg already names the edge."""
    dx = torch.zeros(num_src, dy.shape[1], dtype=dy.dtype, device=dy.device)
    if colidx.numel() == 0 or dy.numel() == 0:
        return dx
    hit = arg >= 0
    src = colidx.to(torch.long)[arg.to(torch.long).clamp(min=0)]
    dx.scatter_add_(0, src, torch.where(hit, dy, torch.zeros_like(dy)))
    return dx


def seg_stats(x: torch.Tensor, rowptr: torch.Tensor, colidx: torch.Tensor,
              num_rows: int, eps: float = 1e-5):
    """The four PNA aggregators of every row's in-neighbourhood.
    Returns (out, stats, arg):
      out   [num_rows, 4*D] = [mean | std | max | min], in x's dtype
      stats [num_rows, 2*D] = [mean | 1/std], unrounded (fp32; fp64 stays)
      arg   [num_rows, 2*D] = [argmax | argmin], int32 forward edge indices
    std = sqrt(var + eps) with the POPULATION variance, computed in two
    passes (the mean first, then the centred squares) on values shifted by
    the row's first edge, so degree-1 rows and rows of equal values have
    var == 0 exactly. max / min and their args are seg_max's (first edge
    wins ties). An empty row gives 0 everywhere and arg -1. NaN and +-inf
    inputs are out of contract."""
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    D = x.shape[1]
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.long)
    dst = torch.repeat_interleave(
        torch.arange(num_rows, dtype=torch.long, device=x.device), deg)
    empty = (deg == 0).unsqueeze(1)
    degc = deg.clamp(min=1).to(ct).unsqueeze(1)
    xc = x.to(ct)
    E = int(colidx.numel())
    zeros = torch.zeros(num_rows, D, dtype=ct, device=x.device)
    if E == 0:
        mean, std, rstd = zeros, zeros, zeros
    else:
        src = colidx.to(torch.long)
        # a trailing empty row starts at E: clamped, then masked
        first = src[rowptr[:-1].to(torch.long).clamp(max=E - 1)]
        x0 = xc[first].masked_fill(empty, 0)
        d = xc[src] - x0[dst]
        m = zeros.index_add(0, dst, d) / degc
        dev = d - m[dst]
        var = zeros.index_add(0, dst, dev * dev) / degc
        mean = x0 + m
        std = torch.sqrt(var + eps)
        rstd = (1.0 / std).masked_fill(empty, 0)
        std = std.masked_fill(empty, 0)
    mx, amx = seg_max(xc, rowptr, colidx, num_rows, "max")
    mn, amn = seg_max(xc, rowptr, colidx, num_rows, "min")
    out = torch.cat([mean, std, mx, mn], 1).to(x.dtype)
    return out, torch.cat([mean, rstd], 1), torch.cat([amx, amn], 1)


def seg_stats_grad(dy: torch.Tensor, x: torch.Tensor, stats: torch.Tensor,
                   arg: torch.Tensor, rowptr: torch.Tensor,
                   colidx: torch.Tensor, num_src: int) -> torch.Tensor:
    """Gradient of seg_stats wrt x from dy [num_rows, 4*D] and the saved
    stats and arg: every edge (u, v) carries
    g_mean[v]/deg_v + g_std[v]*(x[u]-mean[v])*rstd[v]/deg_v, and the max
    and min blocks route whole to their winning edge (seg_max_grad)."""
    ct = stats.dtype
    D = x.shape[1]
    num_rows = dy.shape[0]
    g_mean, g_std, g_max, g_min = (t.to(ct) for t in dy.split(D, 1))
    mean, rstd = stats.split(D, 1)
    amx, amn = arg.split(D, 1)
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.long)
    dst = torch.repeat_interleave(
        torch.arange(num_rows, dtype=torch.long, device=x.device), deg)
    src = colidx.to(torch.long)
    inv = 1.0 / deg.clamp(min=1).to(ct).unsqueeze(1)
    a = g_std * rstd * inv
    term = (g_mean * inv)[dst] + a[dst] * (x.to(ct)[src] - mean[dst])
    dx = torch.zeros(num_src, D, dtype=ct, device=x.device)
    dx.index_add_(0, src, term)
    dx += seg_max_grad(g_max, amx, rowptr, colidx, num_src)
    dx += seg_max_grad(g_min, amn, rowptr, colidx, num_src)
    return dx.to(dy.dtype)


def graph_attention(q: torch.Tensor, kv: torch.Tensor, rowptr: torch.Tensor,
                    colidx: torch.Tensor, num_rows: int, heads: int,
                    scale: float) -> torch.Tensor:
    """Scaled dot-product attention over the in-neighbourhood (PyG's
    TransformerConv without its extras; the reference has no attention):
      s_e = scale * <q[v,h,:], K[u_e,h,:]>   for the edges e of row v
      out[v,h,:] = sum_e softmax_e(s) * V[u_e,h,:]
    q: [num_rows, D], D = heads * dh; kv: [n_src, 2*D] with K in columns
    [0, D) and V in [D, 2D). Duplicate edges each count; a row without
    edges gives 0. Max-subtracted softmax out of index ops, in fp32 (fp64
    stays fp64), differentiable by autograd; the result is cast back to
    q's dtype."""
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    D = q.shape[1]
    dh = D // heads
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.long)
    dst = torch.repeat_interleave(
        torch.arange(num_rows, dtype=torch.long, device=q.device), deg)
    src = colidx.to(torch.long)
    E = int(src.numel())
    qh = q.to(ct).view(num_rows, heads, dh)
    kvh = kv.to(ct).view(kv.shape[0], 2, heads, dh)
    s = (qh[dst] * kvh[src, 0]).sum(dim=2) * scale               # [E, H]
    m = torch.zeros(num_rows, heads, dtype=ct, device=q.device)
    m = m.scatter_reduce(0, dst.unsqueeze(1).expand(E, heads), s.detach(),
                         reduce="amax", include_self=False)
    ex = (s - m[dst]).exp()
    den = torch.zeros(num_rows, heads, dtype=ct,
                      device=q.device).index_add(0, dst, ex)
    alpha = ex / den[dst]
    out = torch.zeros(num_rows, heads, dh, dtype=ct, device=q.device)
    out = out.index_add(0, dst, alpha.unsqueeze(2) * kvh[src, 1])
    return out.reshape(num_rows, D).to(q.dtype)


def _ln_compute_dtype(x: torch.Tensor) -> torch.dtype:
    return torch.float64 if x.dtype == torch.float64 else torch.float32


def layer_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
               eps: float, relu: bool = False):
    """Per-row LayerNorm (+ ReLU) in the kernel's formula
    (`csrc/layer_norm.hip`): mean = sum/D, the CENTRED variance
    sum((x-mean)^2)/D, rstd = 1/sqrt(var+eps),
    y = act((x-mean)*rstd*gamma + beta). Computed in fp32 (fp64 stays
    fp64), y cast back to x's dtype. Returns (y, mean [N], rstd [N]);
    the reference has no normalization layer."""
    ct = _ln_compute_dtype(x)
    D = x.shape[1]
    xf = x.to(ct)
    mean = xf.sum(dim=1) / D
    d = xf - mean.unsqueeze(1)
    var = (d * d).sum(dim=1) / D
    rstd = 1.0 / torch.sqrt(var + eps)
    y = d * rstd.unsqueeze(1) * gamma.to(ct) + beta.to(ct)
    if relu:
        y = torch.relu(y)
    return y.to(x.dtype), mean, rstd


def layer_norm_grad(dy: torch.Tensor, x: torch.Tensor, mean: torch.Tensor,
                    rstd: torch.Tensor, gamma: torch.Tensor,
                    beta: torch.Tensor, relu: bool = False):
    """Gradient of layer_norm from the saved row statistics; xh is
    recomputed, the relu mask is xh*gamma+beta > 0.
      dx = rstd * ((g*gamma - mean_j(g*gamma)) - xh * mean_j(g*gamma*xh))
      dgamma = sum_rows g*xh,  dbeta = sum_rows g
    Returns (dx in x's dtype, dgamma, dbeta in the compute dtype)."""
    ct = _ln_compute_dtype(x)
    D = x.shape[1]
    gam = gamma.to(ct)
    xh = (x.to(ct) - mean.unsqueeze(1)) * rstd.unsqueeze(1)
    g = dy.to(ct)
    if relu:
        g = torch.where(xh * gam + beta.to(ct) > 0, g, torch.zeros_like(g))
    a = g * gam
    m1 = a.sum(dim=1, keepdim=True) / D
    m2 = (a * xh).sum(dim=1, keepdim=True) / D
    dx = rstd.unsqueeze(1) * ((a - m1) - xh * m2)
    return dx.to(x.dtype), (g * xh).sum(dim=0), g.sum(dim=0)


def degnorm(x: torch.Tensor, deg: torch.Tensor) -> torch.Tensor:
    """out[v] = x[v] / sqrt(indeg(v))  (reference `graphnorm_kernel.cu:19-57`)."""
    return x * torch.rsqrt(deg.clamp(min=1.0)).unsqueeze(1).to(x.dtype)


def linear(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """y = x @ w, w stored [in_dim, out_dim] (reference `linear_kernel.cu:76-80`)."""
    return x @ w.to(x.dtype)


def relu(x: torch.Tensor) -> torch.Tensor:
    return torch.relu(x)


def relu_grad(dy: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """dx = dy where y > 0 (reference `linear_kernel.cu:120-127` masks on output)."""
    return dy * (y > 0).to(dy.dtype)


def sigmoid(x: torch.Tensor) -> torch.Tensor:
    return torch.sigmoid(x)


def sigmoid_grad(dy: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    return dy * y * (1.0 - y)


def dropout_mask(shape, p: float, seed: int, offset: int, device) -> torch.Tensor:
    """Deterministic dropout keep-mask from (seed, offset).

    CPU reference for the Philox kernel: uses torch's generator; the HIP
    kernel regenerates its own Philox stream, so GPU-vs-CPU tests compare
    statistics / identity-at-infer, not the exact mask.
    """
    gen = torch.Generator(device="cpu").manual_seed(seed * 0x9E3779B1 + offset)
    return (torch.rand(shape, generator=gen) >= p).to(device)


def softmax_cross_entropy(
    logits: torch.Tensor,
    labels: torch.Tensor,
    mask: torch.Tensor,
    grad_scale: float = 1.0,
    num_classes=None,
):
    """Fused softmax -> CE gradient with train-mask zeroing + metrics.

    Reference `softmax_kernel.cu:19-79`:
      dlogit = softmax(logit) - onehot(label), zeroed where mask != Train
      roc_loss = sum over train rows of (1 - p_true)   (the reference's "loss")
    We additionally report true mean cross-entropy over train rows.
    num_classes < logits width: softmax over the first num_classes cols
    only (padded class dim); pad columns get zero gradient.
    Returns (dlogits, metrics dict).
    """
    stride = logits.shape[1]
    C = num_classes or stride
    if C < stride:
        dl_full = torch.zeros_like(logits)
        dl, md = softmax_cross_entropy(
            logits[:, :C].contiguous(), labels, mask, grad_scale)
        dl_full[:, :C] = dl
        return dl_full, md
    # fp32 accumulation for low-precision inputs (the HIP kernel's
    # behavior); fp32/fp64 inputs keep their own precision (fp64 matters
    # for gradcheck)
    lf = logits if logits.dtype in (torch.float32, torch.float64) \
        else logits.to(torch.float32)
    p = torch.softmax(lf, dim=1)
    n, c = lf.shape
    onehot = torch.zeros_like(p)
    onehot[torch.arange(n, device=lf.device), labels] = 1.0
    train = (mask == MASK_TRAIN)
    dl = (p - onehot) * train.unsqueeze(1).to(p.dtype) * grad_scale
    p_true = p[torch.arange(n, device=lf.device), labels]
    pred = p.argmax(dim=1)
    correct = (pred == labels)
    metrics = {}
    metrics["roc_loss"] = float((1.0 - p_true)[train].sum())
    metrics["ce_loss"] = float((-torch.log(p_true.clamp(min=1e-12))[train]).mean()) if train.any() else 0.0
    for name, m in (("train", MASK_TRAIN), ("val", MASK_VAL), ("test", MASK_TEST)):
        sel = (mask == m)
        metrics[f"{name}_total"] = int(sel.sum())
        metrics[f"{name}_correct"] = int(correct[sel].sum())
    return dl.to(logits.dtype), metrics


def adam_step(
    w: torch.Tensor,
    g: torch.Tensor,
    m: torch.Tensor,
    v: torch.Tensor,
    alpha_t: float,
    beta1: float,
    beta2: float,
    eps: float,
    weight_decay: float,
) -> None:
    """Fused Adam with L2-coupled decay (reference `optimizer_kernel.cu:43-63`):
      gt = g + wd * w;  m,v EMA;  w -= alpha_t * m / (sqrt(v) + eps)
    alpha_t is the bias-corrected step size (reference `optimizer.cc:79-85`).
    In-place on w, m, v.
    """
    gt = g.to(torch.float32) + weight_decay * w
    m.mul_(beta1).add_(gt, alpha=1.0 - beta1)
    v.mul_(beta2).addcmul_(gt, gt, value=1.0 - beta2)
    w.sub_(alpha_t * m / (v.sqrt() + eps))


def glorot_uniform(shape, seed: int) -> torch.Tensor:
    """GlorotUniform: U[-s, s], s = sqrt(6/(in+out))
    (reference `initializer_kernel.cu:22-51`)."""
    fan_in, fan_out = shape[0], shape[1]
    s = (6.0 / (fan_in + fan_out)) ** 0.5
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * s
