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


FP8_MAX = 448.0     # largest e4m3 (OCP, torch.float8_e4m3fn) value
FP8_MIN_EXP = -100  # floor of the row scale's exponent (spmm_fp8.hip)


def quantize_rows_fp8(x: torch.Tensor, pre_scale=None):
    """(q uint8 [N, D], s fp32 [N]) — the bit-exact definition of the GPU
    quantiser (spmm_fp8.hip). y = x * pre_scale in one fp32 multiply;
    s = 2^k with k the smallest integer such that max|y| <= 448 * 2^k
    (k >= FP8_MIN_EXP; s = 1 for an all-zero row); q = RNE_e4m3(y / s), the
    division an exact exponent shift. NaN / inf are out of contract."""
    y = x.float()
    if pre_scale is not None:
        y = y * pre_scale.float().unsqueeze(1)
    amax = y.abs().amax(dim=1)
    m, e = torch.frexp(amax)  # amax = m * 2^e, m in [0.5, 1); 448 = .875 * 2^9
    k = torch.where(m <= 0.875, e - 9, e - 8).clamp(min=FP8_MIN_EXP)
    k = torch.where(amax == 0, torch.zeros_like(k), k)
    s = torch.ldexp(torch.ones_like(amax), k)
    z = torch.ldexp(y, -k.unsqueeze(1)).clamp(-FP8_MAX, FP8_MAX)
    return z.to(torch.float8_e4m3fn).view(torch.uint8), s


def dequantize_rows_fp8(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """fp32 s[r] * decode(q[r, :]); exact, s being a power of two."""
    return q.view(torch.float8_e4m3fn).float() * s.unsqueeze(1)


def spmm_fp8(q: torch.Tensor, s: torch.Tensor, rowptr: torch.Tensor,
             colidx: torch.Tensor, num_rows: int, deg_dst=None,
             out_dtype=torch.bfloat16) -> torch.Tensor:
    """out[v] = deg_dst[v] * sum_e s[u_e] * decode(q[u_e]) as the GPU kernel
    computes it: a sequential fp32 sum in ascending edge order (pass k adds
    edge k of every row that has one), one fp32 multiply by deg_dst, one
    cast."""
    x = dequantize_rows_fp8(q, s)
    deg = rowptr[1:] - rowptr[:-1]
    out = torch.zeros(num_rows, q.shape[1], dtype=torch.float32,
                      device=q.device)
    for k in range(int(deg.max()) if num_rows and colidx.numel() else 0):
        rows = (deg > k).nonzero().squeeze(1)
        out[rows] += x[colidx[rowptr[rows] + k].long()]
    if deg_dst is not None:
        out = out * deg_dst.float().unsqueeze(1)
    return out.to(out_dtype)


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


def seg_softmax(x: torch.Tensor, t: torch.Tensor, rowptr: torch.Tensor,
                colidx: torch.Tensor, num_rows: int):
    """DeeperGCN's softmax aggregation (Li et al. 2020; PyG's GENConv): per
    row v and column j, over the edges e of the row,
      p_e = softmax_e(t * x[u_e, j]),   out[v, j] = sum_e p_e * x[u_e, j]
    with one temperature t (a tensor of one element) for all columns.
    Returns (out, stats): out [num_rows, D] in x's dtype and stats
    [num_rows, 2*D] = [lse | out], unrounded (fp32; fp64 stays), where
    lse = log sum_e exp(t * (x[u_e, j] - out[v, j])), the log-sum-exp of the
    scores centred on the output: it stays of the size of log(deg) where the
    plain one is as large as t * x. The weighted sum is shifted by the
    row's first edge, as seg_stats shifts its sums. Duplicate edges each
    count; an empty row gives 0 everywhere. NaN and +-inf are out of
    contract. The reference has no such aggregator."""
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    D = x.shape[1]
    E = int(colidx.numel())
    zeros = torch.zeros(num_rows, D, dtype=ct, device=x.device)
    if E == 0:
        return zeros.to(x.dtype), torch.cat([zeros, zeros], 1)
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.long)
    dst = torch.repeat_interleave(
        torch.arange(num_rows, dtype=torch.long, device=x.device), deg)
    empty = (deg == 0).unsqueeze(1)
    src = colidx.to(torch.long)
    xs = x.to(ct)[src]                                     # [E, D]
    s = t.to(ct).reshape(()) * xs
    m = zeros.scatter_reduce(0, dst.unsqueeze(1).expand(E, D), s,
                             reduce="amax", include_self=False)
    p = torch.exp(s - m[dst])
    l = zeros.index_add(0, dst, p)
    # a trailing empty row starts at E: clamped, then masked
    x0 = xs[rowptr[:-1].to(torch.long).clamp(max=E - 1)].masked_fill(empty, 0)
    a = zeros.index_add(0, dst, p * (xs - x0[dst]))
    out = (x0 + a / l.clamp(min=1)).masked_fill(empty, 0)
    tc = t.to(ct).reshape(())
    lse = ((m - tc * out) + torch.log(l.clamp(min=1))).masked_fill(empty, 0)
    return out.to(x.dtype), torch.cat([lse, out], 1)


def seg_softmax_grad(dy: torch.Tensor, x: torch.Tensor, stats: torch.Tensor,
                     t: torch.Tensor, rowptr: torch.Tensor,
                     colidx: torch.Tensor, num_src: int):
    """(dx, dt) of seg_softmax from dy [num_rows, D] and the saved stats.
    Every edge (u, v) carries, with d = x[u] - out[v] and
    p = exp(t*d - lse[v]):  dx[u] += p * dy[v] * (1 + t*d),  dt += p * dy[v] * d^2
    (the squared form of sum p*dy*x*d: sum_e p*d = 0, and its terms do not
    cancel). dt is a tensor of one element in stats' dtype."""
    ct = stats.dtype
    D = x.shape[1]
    num_rows = dy.shape[0]
    lse, out = stats.split(D, 1)
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.long)
    dst = torch.repeat_interleave(
        torch.arange(num_rows, dtype=torch.long, device=x.device), deg)
    src = colidx.to(torch.long)
    tc = t.to(ct).reshape(())
    xs = x.to(ct)[src]
    d = xs - out[dst]
    w = torch.exp(tc * d - lse[dst]) * dy.to(ct)[dst]
    dx = torch.zeros(num_src, D, dtype=ct, device=x.device)
    dx.index_add_(0, src, w * (1.0 + tc * d))
    return dx.to(dy.dtype), (w * d * d).sum().reshape(1)


def gated_aggregate(q: torch.Tensor, kv: torch.Tensor, rowptr: torch.Tensor,
                    colidx: torch.Tensor, num_rows: int,
                    normalize: bool = True, eps: float = 1e-6) -> torch.Tensor:
    """Edge-gated aggregation (Bresson & Laurent's residual gated graph
    ConvNet, PyG's ResGatedGraphConv; the reference has no such layer): for
    the edges e = (v <- u_e) of row v and every column j,
      eta[e, j] = sigmoid(q[v, j] + k[u_e, j])
      out[v, j] = sum_e eta[e, j] * val[u_e, j]        / (sum_e eta[e, j] + eps)
    with the division in the mean form (normalize) only. q: [num_rows, D];
    kv: [n_src, 2*D] with k in columns [0, D) and val in [D, 2D). Duplicate
    edges each count; a row without edges gives 0. Index ops in fp32 (fp64
    stays fp64), differentiable by autograd; the result is cast back to q's
    dtype."""
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    D = q.shape[1]
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.long)
    dst = torch.repeat_interleave(
        torch.arange(num_rows, dtype=torch.long, device=q.device), deg)
    src = colidx.to(torch.long)
    k, val = kv.to(ct).split(D, 1)
    eta = torch.sigmoid(q.to(ct)[dst] + k[src])                  # [E, D]
    zeros = torch.zeros(num_rows, D, dtype=ct, device=q.device)
    out = zeros.index_add(0, dst, eta * val[src])
    if normalize:
        out = out / (zeros.index_add(0, dst, eta) + eps)
    return out.to(q.dtype)


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


def gatv2_attention(xl: torch.Tensor, xr: torch.Tensor, att: torch.Tensor,
                    rowptr: torch.Tensor, colidx: torch.Tensor, num_rows: int,
                    heads: int, slope: float = 0.2) -> torch.Tensor:
    """GATv2 dynamic attention over the in-neighbourhood (Brody et al. 2022,
    PyG's GATv2Conv without its extras; the reference has no attention):
      s_e = sum_j att[h,j] * lrelu(xl[u_e,h,j] + xr[v,h,j])  for the edges e
                                                              of row v
      out[v,h,:] = sum_e softmax_e(s) * xl[u_e,h,:]
    xl: [n_src, D], D = heads * dh; xr: [num_rows, D]; att: [heads, dh].
    Duplicate edges each count; a row without edges gives 0. Max-subtracted
    softmax out of index ops, in fp32 (fp64 stays fp64), differentiable by
    autograd; the result is cast back to xr's dtype."""
    ct = torch.float64 if xr.dtype == torch.float64 else torch.float32
    D = xr.shape[1]
    dh = D // heads
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.long)
    dst = torch.repeat_interleave(
        torch.arange(num_rows, dtype=torch.long, device=xr.device), deg)
    src = colidx.to(torch.long)
    E = int(src.numel())
    xlh = xl.to(ct).view(xl.shape[0], heads, dh)
    xrh = xr.to(ct).view(num_rows, heads, dh)
    z = torch.nn.functional.leaky_relu(xlh[src] + xrh[dst], slope)
    s = (z * att.to(ct).unsqueeze(0)).sum(dim=2)                 # [E, H]
    m = torch.zeros(num_rows, heads, dtype=ct, device=xr.device)
    m = m.scatter_reduce(0, dst.unsqueeze(1).expand(E, heads), s.detach(),
                         reduce="amax", include_self=False)
    ex = (s - m[dst]).exp()
    den = torch.zeros(num_rows, heads, dtype=ct,
                      device=xr.device).index_add(0, dst, ex)
    alpha = ex / den[dst]
    out = torch.zeros(num_rows, heads, dh, dtype=ct, device=xr.device)
    out = out.index_add(0, dst, alpha.unsqueeze(2) * xlh[src])
    return out.reshape(num_rows, D).to(xr.dtype)


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


def batch_norm_stats(x: torch.Tensor):
    """Column statistics of [N, D] in the kernel's meaning
    (`csrc/batch_norm.hip`): (mean [D], m2 [D]) with m2 the sum of squared
    deviations, the centred second pass. Zero rows give zeros."""
    ct = _ln_compute_dtype(x)
    xf = x.to(ct)
    if x.shape[0] == 0:
        z = torch.zeros(x.shape[1], dtype=ct, device=x.device)
        return z, z.clone()
    mean = xf.sum(dim=0) / x.shape[0]
    d = xf - mean
    return mean, (d * d).sum(dim=0)


def batch_norm_finalize(mean: torch.Tensor, m2: torch.Tensor, n: int,
                        eps: float, running_mean=None, running_var=None,
                        momentum: float = 0.1) -> torch.Tensor:
    """rstd = 1/sqrt(m2/n + eps) from the (global) mean, m2 and row count.
    Given the running buffers, advances them in place by one step:
    running_var takes the unbiased m2/(n-1) (torch.nn.BatchNorm1d's
    convention) and is left alone at n = 1."""
    rstd = 1.0 / torch.sqrt(m2 / n + eps)
    if running_mean is not None:
        running_mean.mul_(1.0 - momentum).add_(
            momentum * mean.to(running_mean.dtype))
        if n > 1:
            running_var.mul_(1.0 - momentum).add_(
                momentum * (m2 / (n - 1)).to(running_var.dtype))
    return rstd


def batch_norm_apply(x: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor,
                     gamma: torch.Tensor, beta: torch.Tensor,
                     relu: bool = False) -> torch.Tensor:
    """y = act(((x - mean_j) * rstd_j) * gamma_j + beta_j), in x's dtype."""
    ct = _ln_compute_dtype(x)
    y = ((x.to(ct) - mean.to(ct)) * rstd.to(ct)) * gamma.to(ct) + beta.to(ct)
    if relu:
        y = torch.relu(y)
    return y.to(x.dtype)


def batch_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
               running_mean=None, running_var=None, training: bool = True,
               momentum: float = 0.1, eps: float = 1e-5, relu: bool = False):
    """BatchNorm (+ ReLU) over the rows of one rank's [N, D] in the kernels'
    formulas. Training normalises with the batch statistics and advances the
    running buffers in place; eval normalises with the running buffers.
    Returns (y, mean [D], rstd [D]); the reference has no normalization
    layer."""
    if training:
        mean, m2 = batch_norm_stats(x)
        rstd = batch_norm_finalize(mean, m2, x.shape[0], eps, running_mean,
                                   running_var, momentum)
    else:
        mean, rstd = running_mean, 1.0 / torch.sqrt(running_var + eps)
    return batch_norm_apply(x, mean, rstd, gamma, beta, relu), mean, rstd


def batch_norm_bwd_reduce(dy: torch.Tensor, x: torch.Tensor,
                          mean: torch.Tensor, rstd: torch.Tensor,
                          gamma: torch.Tensor, beta: torch.Tensor,
                          relu: bool = False):
    """(dgamma, dbeta) = (sum_rows g*xh, sum_rows g) over this rank's rows;
    xh is recomputed, the relu mask is xh*gamma+beta > 0."""
    ct = _ln_compute_dtype(x)
    xh = (x.to(ct) - mean.to(ct)) * rstd.to(ct)
    g = dy.to(ct)
    if relu:
        g = torch.where(xh * gamma.to(ct) + beta.to(ct) > 0, g,
                        torch.zeros_like(g))
    return (g * xh).sum(dim=0), g.sum(dim=0)


def batch_norm_bwd_dx(dy: torch.Tensor, x: torch.Tensor, mean: torch.Tensor,
                      rstd: torch.Tensor, gamma: torch.Tensor,
                      beta: torch.Tensor, s_g: torch.Tensor,
                      s_gx: torch.Tensor, n: int, relu: bool = False):
    """dx = (gamma*rstd) * ((g - S_g/n) - xh * S_gx/n) from the GLOBAL
    column sums S_g = sum g, S_gx = sum g*xh and the global row count."""
    ct = _ln_compute_dtype(x)
    gam, r = gamma.to(ct), rstd.to(ct)
    xh = (x.to(ct) - mean.to(ct)) * r
    g = dy.to(ct)
    if relu:
        g = torch.where(xh * gam + beta.to(ct) > 0, g, torch.zeros_like(g))
    dx = (gam * r) * ((g - s_g.to(ct) / n) - xh * (s_gx.to(ct) / n))
    return dx.to(x.dtype)


def batch_norm_grad(dy: torch.Tensor, x: torch.Tensor, mean: torch.Tensor,
                    rstd: torch.Tensor, gamma: torch.Tensor,
                    beta: torch.Tensor, relu: bool = False):
    """Training-mode gradient of batch_norm on one rank from the saved
    column statistics. Returns (dx in x's dtype, dgamma, dbeta in the
    compute dtype)."""
    dgamma, dbeta = batch_norm_bwd_reduce(dy, x, mean, rstd, gamma, beta,
                                          relu)
    dx = batch_norm_bwd_dx(dy, x, mean, rstd, gamma, beta, dbeta, dgamma,
                           x.shape[0], relu)
    return dx, dgamma, dbeta


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


PHILOX_FEATURE_STREAM = 0x9E3779B9  # csrc/philox.h: dropout.hip
PHILOX_EDGE_STREAM = 0x7F4A7C15     # csrc/philox.h: spmm_drop.hip


def philox4x32_10(idx, offset: int, seed: int,
                  stream: int = PHILOX_EDGE_STREAM):
    """Philox4x32-10 as csrc/philox.h computes it, in integer arithmetic:
    counter (idx lo, idx hi, offset, stream), key (seed lo, seed hi). idx is
    an array-like of 64-bit counters; returns a uint32 numpy array
    [len(idx), 4], the four output words of each."""
    import numpy as np
    idx = np.asarray(idx).astype(np.uint64).reshape(-1)
    m32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    c0, c1 = idx & m32, idx >> s32
    c2 = np.full_like(c0, int(offset) & 0xFFFFFFFF)
    c3 = np.full_like(c0, int(stream) & 0xFFFFFFFF)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2  # 32 x 32 bits: exact in uint64
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32,
                          (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32)
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def drop_edge_thresh(p: float) -> int:
    """The integer a draw is compared with: min(floor(p * 2^32), 2^32 - 1)."""
    import math
    return min(math.floor(float(p) * 4294967296.0), 0xFFFFFFFF)


def drop_edge_mask(rowptr: torch.Tensor, colidx: torch.Tensor, p: float,
                   seed: int, offset: int,
                   transposed: bool = False) -> torch.Tensor:
    """The DropEdge keep mask of a CSR, bool [E] in its edge order, bit for
    bit the mask of csrc/spmm_drop.hip: edge (v <- u) is kept iff
    philox4x32_10((v << 32) | u, offset, seed).x >= drop_edge_thresh(p), v the
    row and u the column of the forward CSR. transposed=True says the CSR
    given is the transpose (rows are sources): the same function with the
    roles swapped, so no edge permutation is involved. `offset` is the
    effective one (counter * 65536 + offset where a device counter is in
    use), taken modulo 2^32."""
    import numpy as np
    rp = rowptr.cpu().numpy().astype(np.int64)
    row = np.repeat(np.arange(rp.size - 1, dtype=np.uint64),
                    np.diff(rp)).astype(np.uint64)
    col = colidx.cpu().numpy().astype(np.int64).astype(np.uint64)
    v, u = (col, row) if transposed else (row, col)
    draw = philox4x32_10((v << np.uint64(32)) | (u & np.uint64(0xFFFFFFFF)),
                         offset, seed)[:, 0]
    keep = draw.astype(np.uint64) >= np.uint64(drop_edge_thresh(p))
    return torch.from_numpy(keep).to(colidx.device)


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
