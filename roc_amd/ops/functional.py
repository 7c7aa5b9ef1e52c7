"""Autograd operators with HIP-kernel dispatch.

Every op dispatches to the hand-written CDNA4 kernels in ``roc_amd._C``
when the tensors live on a GPU, and to the plain-PyTorch fp32 reference
(`reference.py`) on CPU. There is NO silent eager fallback on GPU: if the
extension is missing for a CUDA tensor, the op raises.

Op semantics follow the reference operator layer;
the architecture (halo-sharded CSR, bf16 activations + fp32 masters,
fused kernels) is MI355X-native.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import reference as ref

try:
    from roc_amd import _C  # built by setup.py build_ext --inplace
except ImportError:  # pragma: no cover - exercised only when ext missing
    _C = None


def has_ext() -> bool:
    return _C is not None


_PHASE_COLS: Optional[int] = None

# -- async dW: the weight-grad GEMMs are independent of the big SpMM^T
# that follows them in backward, and gemm_atb ACCUMULATES (C += the
# split-K partials, folded in a fixed order, all on the launching
# stream), so when the param's .grad buffer exists (flat-grad setup)
# the dW launches on a side stream and lands directly in .grad while
# the aggregation backward runs. dw_flush() joins the side stream
# before any gradient consumer (all-reduce / Adam).
# Default OFF by measurement (profiles/r29 addendum): the epoch is
# memory-saturated end-to-end, so overlapping the memory-bound dW with
# the memory-bound SpMM^T returns nothing (15.88 vs 15.83 ms sync) —
# the capability stays for compute-bound model mixes (ROC_ASYNC_DW=1).
_DW_STREAM = None
_DW_PENDING: list = []  # [(done_event, (x, dy) keep-alive refs)]
_ASYNC_DW: Optional[bool] = None


def _async_dw() -> bool:
    global _ASYNC_DW
    if _ASYNC_DW is None:
        import os
        _ASYNC_DW = os.environ.get("ROC_ASYNC_DW", "0") == "1"
    return _ASYNC_DW


def _dw_stream():
    global _DW_STREAM
    if _DW_STREAM is None:
        _DW_STREAM = torch.cuda.Stream()
    return _DW_STREAM


def dw_flush() -> None:
    """Make the current stream wait for every pending side-stream dW
    GEMM. Call before anything that reads or zeroes gradients."""
    if not _DW_PENDING:
        return
    from .. import streamcheck
    cs = torch.cuda.current_stream()
    for done, _refs in _DW_PENDING:
        streamcheck.consumer(done, "dw-consume")
        cs.wait_event(done)
    _DW_PENDING.clear()


def _phase_cols() -> int:
    """Column-phase width for strip-blocked SpMM passes (0 = off).

    Default OFF by measurement (profiles/r23): at equal gather
    working-set bytes, 64-col phases run the headline epoch 19.4 ms vs
    16.0 ms single-phase — narrow 128-B row gathers pay a ~20% service
    penalty vs whole 512-B rows, and the partial-traffic saving never
    lands because phases multiply the pass count right back.
    Pinned at first use for the same reason the kernel geometry knobs
    are: a per-launch getenv on the hot path silently desyncs from any
    hipGraph capture.
    """
    global _PHASE_COLS
    if _PHASE_COLS is None:
        import os
        _PHASE_COLS = int(os.environ.get("ROC_SPMM_PHASE_COLS", "0"))
    return _PHASE_COLS


def _hip(x: torch.Tensor) -> bool:
    if x.is_cuda:
        if _C is None:
            raise RuntimeError(
                "roc_amd._C extension is not built but a GPU tensor was passed. "
                "Run `python setup.py build_ext --inplace`. Refusing a silent "
                "eager fallback on GPU."
            )
        return True
    return False


# ---------------------------------------------------------------------------
# ScatterGather (CSR SpMM neighbor aggregation) — the hot op
# ---------------------------------------------------------------------------

def _order_applies(x) -> bool:
    """The ordered plan serves whole-row bf16 passes only. The shard holds
    no natural plan next to it, so every other caller (fp32, D % 8 != 0,
    column phases) takes the one-pass kernel on the full CSR — the same
    fp32 adds in the same order."""
    return (x.dtype == torch.bfloat16 and x.shape[1] % 8 == 0
            and not _phase_cols())


def _spmm_launcher(fp8_scale):
    """_C.spmm, or for e4m3 rows _C.spmm_fp8 bound to their scales behind
    _C.spmm's positional signature, so one strip driver serves both."""
    if fp8_scale is None:
        return _C.spmm

    def run(out, q, rowptr, colidx, deg_dst=None, deg_src=None,
            row_order=None, accumulate=False, col_base=0, ncols=0,
            heavy_rows=None, heavy_min=0, final_out=None, out_rows=None,
            relu=False, post_scale=None):
        assert deg_src is None and col_base == 0 and ncols == 0
        assert not relu and post_scale is None, \
            "fp8 passes have no store epilogues"
        _C.spmm_fp8(out, q, fp8_scale, rowptr, colidx, deg_dst, row_order,
                    accumulate, heavy_rows, heavy_min, final_out, out_rows)
    return run


def _strip_spmm_ordered(x, strips, num_rows, row_scale, order,
                        fp8_scale=None, relu=False, post_scale=None):
    """The strip SpMM on a degree-ordered plan
    (partition.build_strip_plan_ordered): the light rows in one plain
    pass, then the heavy region's K-1 accumulate passes over fp32 partials
    kept in plan order, then its final pass; the light and the final pass
    store their bf16 rows through the plan's permutation into one out.
    relu / post_scale ride those two stores (see _strip_spmm)."""
    perm_heavy, perm_light, lrp, lci = order
    epi = (relu, post_scale) if relu or post_scale is not None else ()
    D = x.shape[1]
    spmm = _spmm_launcher(fp8_scale)
    out = torch.empty(num_rows, D, dtype=torch.bfloat16, device=x.device)
    if perm_light.numel():
        spmm(out, x, lrp, lci, row_scale, None, None, False, 0, 0, None,
             0, None, perm_light, *epi)
    n_heavy = perm_heavy.numel()
    if n_heavy:
        out32 = torch.empty(n_heavy, D, dtype=torch.float32, device=x.device)
        last = len(strips) - 1
        for i, (srp, sci) in enumerate(strips):
            if i < last:
                spmm(out32, x, srp, sci, None, None, None, i > 0)
            else:
                spmm(out32, x, srp, sci, row_scale, None, None, i > 0,
                     0, 0, None, 0, out, perm_heavy, *epi)
    return out


def _strip_spmm(x, strips, num_rows, row_scale, heavy=None, heavy_min=0,
                order=None, fp8_scale=None, relu=False, post_scale=None):
    """Source-strip-blocked SpMM: each pass gathers from an L2-resident
    source window; partials accumulate in fp32 (one rounding total —
    same numerics as single-pass). Wide feature dims additionally sweep
    column PHASES: a 64-col phase over 4x-wider strips keeps the same
    gather working set (rows x cols bytes) while the fp32 partial buffer
    is re-read/re-written 4x less often — partial traffic, not gathers,
    was the next bound (profiles/r23). The epilogue casts back to
    x.dtype and applies the optional fp32 row_scale; for bf16 the last
    whole-row pass does that itself (final_out) and no cast pass runs.
    heavy: per-strip heavy-first row lists with their threshold
    (partition.build_strip_heavy), bf16 passes only.
    order: the strips are a degree-ordered plan (_strip_spmm_ordered).
    fp8_scale: x is the e4m3 bytes of quantize_rows_fp8 and this its scale
    vector; the passes are the bf16 whole-row ones on the fp8 kernel (no
    column phases: the caller takes the one-pass kernel when they are on).
    relu: the result is max(0, .) of the scaled sum. post_scale: a second
    fp32 row factor applied to the *stored* result, that is rounded twice,
    exactly as a rowscale pass over the output would. Both ride the store of
    the last bf16 pass; the other epilogues run them as passes of their own."""
    fp8 = fp8_scale is not None
    epi = (relu, post_scale) if relu or post_scale is not None else ()
    assert not (fp8 and _phase_cols()), "fp8 strip passes: whole rows only"
    if order is not None:
        assert fp8 or _order_applies(x), \
            "ordered strip plan: whole-row bf16 only"
        return _strip_spmm_ordered(x, strips, num_rows, row_scale, order,
                                   fp8_scale, relu, post_scale)
    spmm = _spmm_launcher(fp8_scale)
    D = x.shape[1]
    out32 = torch.empty(num_rows, D, dtype=torch.float32, device=x.device)
    ph = _phase_cols()
    if ph and D % ph == 0 and D // ph >= 2:
        phases = [(p, ph) for p in range(0, D, ph)]
    else:
        phases = [(0, 0)]  # one whole-row phase
    bf16 = x.dtype == torch.bfloat16 or fp8  # the result is bf16
    fuse_final = bf16 and D % 8 == 0 and phases == [(0, 0)]
    if not bf16:
        heavy = None
    out = None
    for col_base, ncols in phases:
        for i, (srp, sci) in enumerate(strips):
            hv = heavy[i] if heavy is not None else None
            if fuse_final and i == len(strips) - 1:
                out = torch.empty(num_rows, D, dtype=torch.bfloat16,
                                  device=x.device)
                spmm(out32, x, srp, sci, row_scale, None, None, i > 0,
                     0, 0, hv, heavy_min, out, None, *epi)
            else:
                spmm(out32, x, srp, sci, None, None, None, i > 0,
                     col_base, ncols, hv, heavy_min)
    if out is not None:
        return out
    if x.dtype == torch.bfloat16 and D % 8 == 0:
        out = torch.empty(num_rows, D, dtype=torch.bfloat16, device=x.device)
        _C.cast_rowscale(out, out32, row_scale)  # fused epilogue
    else:
        if row_scale is not None:
            out32 = out32 * row_scale.unsqueeze(1)
        out = out32.to(x.dtype)
    if relu:  # the maps take restrict pointers: never in place
        act = torch.empty_like(out)
        _C.relu_fwd(act, out)
        out = act
    if post_scale is not None:
        scaled = torch.empty_like(out)
        _C.rowscale(scaled, out, post_scale)
        out = scaled
    return out


class _SpMM(torch.autograd.Function):
    """out[v] = sum over in-neighbors of x[u] on a (possibly halo-extended,
    possibly degree-normalized) local CSR. Backward runs the same kernel on
    the transpose CSR (exact on asymmetric graphs)."""

    @staticmethod
    def forward(ctx, x, rowptr, colidx, t_rowptr, t_colidx, num_rows, num_ext,
                deg_dst, deg_src, row_order, t_row_order,
                fwd_strips=None, bwd_strips=None, fwd_heavy=None,
                bwd_heavy=None, heavy_min=0, fwd_order=None, bwd_order=None,
                relu=False, grad_src_scale=None, bwd_loss=None):
        # relu: out = max(0, .), and the backward masks dy by it.
        # grad_src_scale: fp32 [num_ext], multiplied into the stored dx the
        # way a rowscale pass over it would (the consumer's own backward
        # row scaling, handed over).
        # bwd_loss: (strips, heavy, keep) of GraphShard.install_loss_rows;
        # the caller guarantees dy is zero outside keep.
        ctx.num_ext = num_ext
        ctx.bwd_strips = bwd_strips
        ctx.bwd_heavy = (bwd_heavy, heavy_min, bwd_order)
        ctx.bwd_loss = bwd_loss
        ctx.relu = relu
        if (_hip(x) and fwd_strips is not None and deg_src is None
                and (fwd_order is None or _order_applies(x))):
            out = _strip_spmm(x, fwd_strips, num_rows, deg_dst, fwd_heavy,
                              heavy_min, fwd_order, relu=relu)
        elif _hip(x):
            out = torch.empty(num_rows, x.shape[1], dtype=x.dtype, device=x.device)
            fuse = relu and deg_src is None
            _C.spmm(out, x, rowptr, colidx, deg_dst, deg_src, row_order,
                    relu=fuse)
            if relu and not fuse:
                act = torch.empty_like(out)
                _C.relu_fwd(act, out)
                out = act
        else:
            xin = x
            if deg_src is not None:  # deg_* are precomputed row scale factors
                xin = xin * deg_src.unsqueeze(1).to(xin.dtype)
            out = ref.spmm(xin, rowptr, colidx, num_rows)
            if deg_dst is not None:
                out = out * deg_dst.unsqueeze(1).to(out.dtype)
            if relu:
                out = ref.relu(out)
        ctx.save_for_backward(t_rowptr, t_colidx, deg_dst, deg_src,
                              t_row_order, grad_src_scale,
                              out if relu else None)
        return out

    @staticmethod
    def backward(ctx, dy):
        (t_rowptr, t_colidx, deg_dst, deg_src, t_row_order, gss,
         y) = ctx.saved_tensors
        dy = dy.contiguous()
        # d/dx of  diag(a) A diag(b) x  =  diag(b) A^T diag(a) dy
        if _hip(dy):
            if ctx.relu:
                # the ReLU mask and the pre-scale below in one pass
                tmp = torch.empty_like(dy)
                _C.relu_bwd(tmp, dy, y, deg_dst)
                dy = tmp
            elif deg_dst is not None:
                # pre-scale the gradient rows ONCE (one cheap pass) instead
                # of a per-edge deg gather inside the transpose SpMM
                tmp = torch.empty_like(dy)
                _C.rowscale(tmp, dy, deg_dst)
                dy = tmp
            if ctx.bwd_strips is not None and deg_src is None \
                    and ctx.bwd_loss is not None:
                strips, heavy, keep = ctx.bwd_loss
                _debug_check_loss_rows(dy, keep)
                dx = _strip_spmm(dy, strips, ctx.num_ext, None, heavy,
                                 ctx.bwd_heavy[1], post_scale=gss)
            elif (ctx.bwd_strips is not None and deg_src is None
                    and (ctx.bwd_heavy[2] is None or _order_applies(dy))):
                dx = _strip_spmm(dy, ctx.bwd_strips, ctx.num_ext, None,
                                 *ctx.bwd_heavy, post_scale=gss)
            else:
                dx = torch.empty(ctx.num_ext, dy.shape[1], dtype=dy.dtype,
                                 device=dy.device)
                fuse = gss if deg_src is None else None
                _C.spmm(dx, dy, t_rowptr, t_colidx, deg_src, None, t_row_order,
                        post_scale=fuse)
                if gss is not None and fuse is None:
                    scaled = torch.empty_like(dx)
                    _C.rowscale(scaled, dx, gss)
                    dx = scaled
        else:
            yin = dy
            if ctx.relu:
                yin = ref.relu_grad(yin, y)
            if deg_dst is not None:
                yin = yin * deg_dst.unsqueeze(1).to(yin.dtype)
            dx = ref.spmm(yin, t_rowptr, t_colidx, ctx.num_ext)
            if deg_src is not None:
                dx = dx * deg_src.unsqueeze(1).to(dx.dtype)
            if gss is not None:
                dx = dx * gss.unsqueeze(1).to(dx.dtype)
        return (dx,) + (None,) * 20


_DEBUG_LOSS_ROWS = None


def _debug_check_loss_rows(dy, keep) -> None:
    """ROC_DEBUG_LOSS_ROWS=1: before a pruned transpose plan is used, check
    what its caller guarantees, that dy is zero on every row outside the
    keep-vector. A violation would silently lose gradient. Eager only: the
    check reads the device, so it never runs under stream capture."""
    global _DEBUG_LOSS_ROWS
    if _DEBUG_LOSS_ROWS is None:
        import os
        _DEBUG_LOSS_ROWS = os.environ.get("ROC_DEBUG_LOSS_ROWS", "0") == "1"
    if not _DEBUG_LOSS_ROWS or torch.cuda.is_current_stream_capturing():
        return
    bad = (dy[~keep] != 0).any(dim=1)
    if bool(bad.any()):
        raise RuntimeError(
            f"loss_rows_only: {int(bad.sum())} gradient rows outside the "
            "shard's loss rows are nonzero")


def quantize_rows_fp8(x, pre_scale=None):
    """(q, s): the rows of bf16 x, times the fp32 row factor pre_scale if
    given, as e4m3 bytes (uint8 [N, D]) and one power-of-two fp32 scale per
    row, so that x[r] * pre_scale[r] ~= s[r] * decode(q[r]) to one e4m3
    rounding per element. D must be a multiple of 16, at most 1024. GPU:
    spmm_fp8.hip, no host read and no sync; CPU: ops.reference, the same
    bits."""
    if x.dim() != 2 or x.dtype != torch.bfloat16:
        raise ValueError("quantize_rows_fp8: x must be a bf16 [N, D] matrix, "
                         f"got {x.dtype} {tuple(x.shape)}")
    if x.shape[1] % 16 != 0 or not 16 <= x.shape[1] <= 1024:
        raise ValueError("quantize_rows_fp8: D must be a multiple of 16 in "
                         f"[16, 1024], got {x.shape[1]}")
    if not _hip(x):
        return ref.quantize_rows_fp8(x, pre_scale)
    x = x.contiguous()
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    s = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    _C.quantize_rows_fp8(q, s, x, pre_scale)
    return q, s


def _spmm_fp8(x, pre_scale, rowptr, colidx, num_rows, row_scale, row_order,
              strips, heavy, heavy_min, order):
    """diag(row_scale) A diag(pre_scale) x with the rows of x gathered as
    e4m3: quantise (pre_scale folded in), then the fp8 SpMM on the strip
    plan if there is one, else the one-pass kernel. bf16 in, bf16 out."""
    q, s = quantize_rows_fp8(x, pre_scale)
    if not _hip(x):
        return ref.spmm_fp8(q, s, rowptr, colidx, num_rows, row_scale)
    if strips is not None and not _phase_cols():
        return _strip_spmm(q, strips, num_rows, row_scale, heavy, heavy_min,
                           order, fp8_scale=s)
    out = torch.empty(num_rows, x.shape[1], dtype=torch.bfloat16,
                      device=x.device)
    _C.spmm_fp8(out, q, s, rowptr, colidx, row_scale, row_order)
    return out


class _SpMMFp8(torch.autograd.Function):
    """_SpMM with every gathered row in e4m3 (gather_dtype="fp8"): the
    forward quantises x (deg_src folded into the quantiser), the backward
    quantises dy (deg_dst folded in) and is straight-through in x. The other
    degree factor is applied in fp32 at the store. Same arguments as _SpMM."""

    @staticmethod
    def forward(ctx, x, rowptr, colidx, t_rowptr, t_colidx, num_rows, num_ext,
                deg_dst, deg_src, row_order, t_row_order,
                fwd_strips=None, bwd_strips=None, fwd_heavy=None,
                bwd_heavy=None, heavy_min=0, fwd_order=None, bwd_order=None):
        ctx.save_for_backward(t_rowptr, t_colidx, deg_dst, deg_src, t_row_order)
        ctx.num_ext = num_ext
        ctx.bwd_plan = (bwd_strips, bwd_heavy, heavy_min, bwd_order)
        return _spmm_fp8(x, deg_src, rowptr, colidx, num_rows, deg_dst,
                         row_order, fwd_strips, fwd_heavy, heavy_min,
                         fwd_order)

    @staticmethod
    def backward(ctx, dy):
        t_rowptr, t_colidx, deg_dst, deg_src, t_row_order = ctx.saved_tensors
        dx = _spmm_fp8(dy.contiguous(), deg_dst, t_rowptr, t_colidx,
                       ctx.num_ext, deg_src, t_row_order, *ctx.bwd_plan)
        return (dx,) + (None,) * 17


def _edge_call_offset(call_id):
    """(seed, offset, counter) of one mask draw, taken from the dropout
    state exactly as _Dropout takes them: a call_id gives a stable per-epoch
    offset (identical on a recompute re-forward; the epoch comes from the
    device counter under hipGraph, else from the host), no call_id takes
    the running offset."""
    counter = _DROPOUT_STATE["counter"]
    if call_id is not None:
        offset = int(call_id)
        if counter is None:
            offset += _DROPOUT_STATE["epoch"] * 65536
    else:
        offset = _DROPOUT_STATE["offset"]
        _DROPOUT_STATE["offset"] += 1
    return _DROPOUT_STATE["seed"], offset, counter


def _spmm_drop(x, rowptr, colidx, num_rows, pre_scale, row_scale, row_order,
               p, seed, offset, counter, transposed):
    """diag(row_scale) / (1 - p) * (A o mask) diag(pre_scale) x over one CSR
    (transposed: the transpose CSR, the same mask). GPU: one rowscale pass
    for pre_scale, then spmm_drop.hip; CPU: the reference mask and spmm."""
    if _hip(x):
        x = x.contiguous()
        if pre_scale is not None:
            tmp = torch.empty_like(x)
            _C.rowscale(tmp, x, pre_scale)
            x = tmp
        out = torch.empty(num_rows, x.shape[1], dtype=x.dtype, device=x.device)
        _C.spmm_drop(out, x, rowptr, colidx, p, seed, offset, counter,
                     row_scale, row_order, transposed)
        return out
    if counter is not None:
        offset += int(counter.item()) * 65536
    keep = ref.drop_edge_mask(rowptr, colidx, p, seed, offset, transposed)
    if pre_scale is not None:
        x = x * pre_scale.unsqueeze(1).to(x.dtype)
    out = ref.spmm_weighted(x, rowptr, colidx, keep.to(x.dtype), num_rows)
    if row_scale is not None:
        out = out * row_scale.unsqueeze(1).to(out.dtype)
    return out * (1.0 / (1.0 - p))


class _SpMMDrop(torch.autograd.Function):
    """_SpMM over the edges a stateless DropEdge mask keeps, scaled by
    1 / (1 - p). The mask is a pure function of (seed, offset, counter, v, u)
    (spmm_drop.hip), so nothing is stored: the backward runs the same kernel
    on the transpose CSR and draws the same mask with the roles swapped."""

    @staticmethod
    def forward(ctx, x, rowptr, colidx, t_rowptr, t_colidx, num_rows, num_ext,
                deg_dst, deg_src, row_order, t_row_order, p, call_id):
        ctx.save_for_backward(t_rowptr, t_colidx, deg_dst, deg_src, t_row_order)
        ctx.num_ext = num_ext
        ctx.draw = (p,) + _edge_call_offset(call_id)
        return _spmm_drop(x, rowptr, colidx, num_rows, deg_src, deg_dst,
                          row_order, *ctx.draw, False)

    @staticmethod
    def backward(ctx, dy):
        t_rowptr, t_colidx, deg_dst, deg_src, t_row_order = ctx.saved_tensors
        dx = _spmm_drop(dy.contiguous(), t_rowptr, t_colidx, ctx.num_ext,
                        deg_dst, deg_src, t_row_order, *ctx.draw, True)
        return (dx,) + (None,) * 12


def scatter_gather_drop_csr(x, rowptr, colidx, t_rowptr, t_colidx, num_rows,
                            num_ext, p, dst_scale=None, src_scale=None,
                            row_order=None, t_row_order=None, call_id=None):
    """_SpMMDrop over an explicit CSR pair (parallel.aggregate runs it over
    the gather-space CSR of allgather mode)."""
    if not 0.0 < p < 1.0:
        raise ValueError(f"edge_drop must be in (0, 1), got {p}")
    return _SpMMDrop.apply(x, rowptr, colidx, t_rowptr, t_colidx, num_rows,
                           num_ext, dst_scale, src_scale, row_order,
                           t_row_order, float(p), call_id)


class _SpMMEdge(torch.autograd.Function):
    """out[v] = sum_{e in row v} w[e] * x[col_e]  (+ optional dst row
    scale). The edge-tensor consumer op: w is a per-local-edge tensor
    in CSR edge order (the reference declares edge tensors,
    `gnn.cc:475-623`, but ships no op over them — this makes the
    surface real). Backward: dx rides the transpose CSR with permuted
    weights; dw[e] = <dy[row_e], x[col_e]>."""

    @staticmethod
    def forward(ctx, x, w, rowptr, colidx, t_rowptr, t_colidx, t_eperm,
                num_rows, num_ext, dst_scale, row_order, t_row_order):
        w = w.contiguous()
        ctx.save_for_backward(x, w, rowptr, colidx, t_rowptr, t_colidx,
                              t_eperm, dst_scale, t_row_order)
        ctx.num_ext = num_ext
        if _hip(x):
            out = torch.empty(num_rows, x.shape[1], dtype=x.dtype,
                              device=x.device)
            _C.spmm_edge(out, x, rowptr, colidx, w, dst_scale, row_order,
                         False)
        else:
            out = ref.spmm_weighted(x, rowptr, colidx, w, num_rows)
            if dst_scale is not None:
                out = out * dst_scale.unsqueeze(1).to(out.dtype)
        return out

    @staticmethod
    def backward(ctx, dy):
        (x, w, rowptr, colidx, t_rowptr, t_colidx, t_eperm, dst_scale,
         t_row_order) = ctx.saved_tensors
        dy = dy.contiguous()
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx = dw = None
        if _hip(dy):
            if dst_scale is not None:
                tmp = torch.empty_like(dy)
                _C.rowscale(tmp, dy, dst_scale)
                dy = tmp
            if need_x:
                t_w = w[t_eperm].contiguous()
                dx = torch.empty(ctx.num_ext, dy.shape[1], dtype=dy.dtype,
                                 device=dy.device)
                _C.spmm_edge(dx, dy, t_rowptr, t_colidx, t_w, None,
                             t_row_order, False)
            if need_w:
                dw = torch.empty_like(w)
                _C.edge_dot(dw, dy, x, rowptr, colidx)
        else:
            if dst_scale is not None:
                dy = dy * dst_scale.unsqueeze(1).to(dy.dtype)
            if need_x:
                dx = ref.spmm_weighted(dy, t_rowptr, t_colidx, w[t_eperm],
                                       ctx.num_ext)
            if need_w:
                dw = ref.edge_dot(dy, x, rowptr, colidx).to(w.dtype)
        return (dx, dw) + (None,) * 10


def scatter_gather_weighted(x, w, shard, dst_scale=None):
    """Per-edge-weighted neighbor aggregation over the shard's local CSR.

    x: [n_ext, D] halo-extended features; w: fp32 [num_local_edges] in
    CSR edge order (see roc_amd.edge_tensor). Returns [n_local, D].
    Both x and w receive gradients. Works at any world size — edge
    tensors are partition-local, so no extra communication beyond the
    usual halo exchange of x."""
    return _SpMMEdge.apply(
        x, w, shard.rowptr, shard.colidx, shard.t_rowptr, shard.t_colidx,
        shard.t_edge_perm(), shard.n_local, shard.n_ext, dst_scale,
        shard.row_order, shard.t_row_order)


class _EdgeSoftmax(torch.autograd.Function):
    """Per-destination-row segment softmax over edge scores (the GAT
    attention normalizer). GPU: one fused CDNA4 kernel per direction
    (edge_softmax.hip); CPU: index-op reference."""

    @staticmethod
    def forward(ctx, s, rowptr, row_of_edge):
        s = s.contiguous()
        if _hip(s):
            alpha = torch.empty_like(s)
            _C.edge_softmax_fwd(alpha, s, rowptr)
        else:
            n = rowptr.numel() - 1
            m = torch.full((n,), float("-inf"), dtype=s.dtype)
            m = m.scatter_reduce(0, row_of_edge, s, reduce="amax",
                                 include_self=True)
            ex = (s - m[row_of_edge]).exp()
            denom = torch.zeros(n, dtype=s.dtype).index_add_(
                0, row_of_edge, ex)
            alpha = ex / denom[row_of_edge]
        ctx.save_for_backward(alpha, rowptr, row_of_edge)
        return alpha

    @staticmethod
    def backward(ctx, dalpha):
        alpha, rowptr, row_of_edge = ctx.saved_tensors
        dalpha = dalpha.contiguous()
        if _hip(dalpha):
            ds = torch.empty_like(dalpha)
            _C.edge_softmax_bwd(ds, dalpha, alpha, rowptr)
        else:
            n = rowptr.numel() - 1
            dot = torch.zeros(n, dtype=alpha.dtype).index_add_(
                0, row_of_edge, alpha * dalpha)
            ds = alpha * (dalpha - dot[row_of_edge])
        return ds, None, None


def edge_softmax(scores, shard):
    """softmax of fp32 edge scores within each destination row's
    in-edge segment: Σ_{e∈row v} out[e] = 1. Differentiable; pairs
    with scatter_gather_weighted for attention-style aggregation."""
    return _EdgeSoftmax.apply(scores.float(), shard.rowptr,
                              shard.row_of_edge())


class _AttentionSoftmax(torch.autograd.Function):
    """alpha[e] = softmax_row(lrelu(s_src[col_e] + s_dst[row])) — the
    whole GAT score+normalize chain in ONE kernel per direction
    (edge_softmax.hip att_*). Replaces 4 E-length torch intermediates
    and a 115M-element index_add backward. CPU path composes index
    ops (the numerics oracle)."""

    @staticmethod
    def forward(ctx, s_src, s_dst, rowptr, colidx, row_of_edge, slope):
        s_src = s_src.contiguous()
        s_dst = s_dst.contiguous()
        if _hip(s_src):
            alpha = torch.empty(colidx.numel(), dtype=torch.float32,
                                device=s_src.device)
            _C.att_softmax_fwd(alpha, s_src, s_dst, rowptr, colidx, slope)
        else:
            n = rowptr.numel() - 1
            sc = s_src[colidx.long()] + s_dst[row_of_edge]
            sc = torch.nn.functional.leaky_relu(sc, slope)
            m = torch.full((n,), float("-inf"), dtype=sc.dtype)
            m = m.scatter_reduce(0, row_of_edge, sc, reduce="amax",
                                 include_self=True)
            ex = (sc - m[row_of_edge]).exp()
            den = torch.zeros(n, dtype=sc.dtype).index_add_(
                0, row_of_edge, ex)
            alpha = ex / den[row_of_edge]
        ctx.save_for_backward(alpha, s_src, s_dst, rowptr, colidx,
                              row_of_edge)
        ctx.slope = slope
        return alpha

    @staticmethod
    def backward(ctx, dalpha):
        alpha, s_src, s_dst, rowptr, colidx, row_of_edge = ctx.saved_tensors
        slope = ctx.slope
        dalpha = dalpha.contiguous()
        if _hip(dalpha):
            dsrc = torch.zeros_like(s_src)
            dsdst = torch.empty_like(s_dst)
            _C.att_softmax_bwd(dsrc, dsdst, dalpha, alpha, s_src, s_dst,
                               rowptr, colidx, slope)
        else:
            n = rowptr.numel() - 1
            dot = torch.zeros(n, dtype=alpha.dtype).index_add_(
                0, row_of_edge, alpha * dalpha)
            ds = alpha * (dalpha - dot[row_of_edge])
            raw = s_src[colidx.long()] + s_dst[row_of_edge]
            dscore = torch.where(raw > 0, ds, slope * ds)
            dsrc = torch.zeros_like(s_src).index_add_(
                0, colidx.long(), dscore)
            dsdst = torch.zeros_like(s_dst).index_add_(
                0, row_of_edge, dscore)
        return dsrc, dsdst, None, None, None, None


def attention_softmax(s_src, s_dst, shard, slope: float = 0.2):
    """Fused GAT attention coefficients from per-node score halves:
    s_src fp32 [n_ext] (source half, halo-extended), s_dst fp32
    [n_local]. Returns alpha fp32 [E_local]; both inputs get grads."""
    return _AttentionSoftmax.apply(s_src.float(), s_dst.float(),
                                   shard.rowptr, shard.colidx,
                                   shard.row_of_edge(), slope)


def scatter_gather(x, shard, normalize: bool = False, dst_scale=None,
                   src_scale=None, gather_dtype=None, edge_drop: float = 0.0,
                   training: bool = False, edge_call_id=None,
                   relu: bool = False, grad_src_scale=None,
                   loss_rows_only: bool = False):
    """Neighbor sum-aggregation over the shard's local CSR.

    x: [n_ext, D] halo-extended features. Returns [n_local, D].
    normalize=True fuses the symmetric D^-1/2 A D^-1/2 GCN normalization
    (the reference composes indegree_norm -> scatter_gather -> indegree_norm,
    `gnn.cc:82-84`; the fused kernel reads each feature once instead).
    dst_scale/src_scale: explicit per-row fp32 factors. The fast GCN path
    pre-scales sources in the linear epilogue and passes only dst_scale
    here (saves one gather per edge).
    gather_dtype="fp8" gathers every row as OCP e4m3 with one power-of-two
    scale per row (spmm_fp8.hip): half the bytes per gathered row, fp32
    accumulation, one e4m3 rounding per gathered element, in the forward
    (x) and in the backward (dy, straight-through in x). It needs bf16 x
    with D % 16 == 0, D <= 1024, and raises otherwise. The default,
    shard.gather_dtype, is a preference instead: a call whose x is not bf16
    or whose width does not qualify runs the bf16 path. Measured on the
    Reddit shape (profiles/r46) it is no faster: D = 256 forward +10%,
    forward + backward even; D = 64 loses clearly (4.1 against 2.1 ms
    forward). It is opt-in; docs/KERNELS.md, spmm_fp8, has the table.
    edge_drop=p with training=True is DropEdge (Rong et al., ICLR 2020): each
    edge is dropped with probability p by a stateless mask drawn inside the
    gather kernel (spmm_drop.hip), and the sum over the kept edges is scaled
    by 1 / (1 - p); the degree factors stay those of the full graph. The mask
    takes seed, epoch and device counter from the dropout state as
    dropout() does, with edge_call_id in the place of call_id (the models
    pass the layer index), so it is identical on a recompute re-forward and
    fresh on every epoch and hipGraph replay; the backward redraws it.
    edge_drop == 0 or training false is the undropped path, untouched. The
    drop path always runs its one-pass kernel on the full CSR: strip plans
    are not used with it (a strip plan of the drop kernel is the follow-up),
    and it does not combine with gather_dtype="fp8" (raises; a shard-level
    fp8 preference gives way). docs/KERNELS.md, spmm_drop, has the numbers.
    relu=True returns max(0, .) of the result, in the store of the SpMM, and
    the backward masks the gradient by it (with the dst pre-scale, one pass).
    grad_src_scale: fp32 [n_ext]; the gradient w.r.t. x comes back multiplied
    by it per row, rounded as a rowscale pass over the stored gradient would
    round (the producer of x then skips that pass: linear(grad_prescaled=
    True)). loss_rows_only=True is the caller's promise that the incoming
    gradient is zero outside the rows the shard's loss-row plan was built
    for (GraphShard.install_loss_rows); the backward then skips those
    columns of the transpose. Without such a plan it changes nothing. All
    three belong to the plain bf16/fp32 path: the DropEdge and fp8 paths
    take none of them (relu / grad_src_scale raise there).
    """
    deg_dst = shard.rsqrt_deg_local if normalize else dst_scale
    deg_src = shard.rsqrt_deg_ext if normalize else src_scale
    if training and edge_drop > 0.0:
        if gather_dtype == "fp8":
            raise ValueError("scatter_gather: edge_drop > 0 does not combine "
                             "with gather_dtype='fp8'")
        if relu or grad_src_scale is not None:
            raise ValueError("scatter_gather: relu / grad_src_scale do not "
                             "combine with edge_drop")
        return scatter_gather_drop_csr(
            x, shard.rowptr, shard.colidx, shard.t_rowptr, shard.t_colidx,
            shard.n_local, shard.n_ext, edge_drop, deg_dst, deg_src,
            shard.row_order, shard.t_row_order, edge_call_id)
    fits = (x.dtype == torch.bfloat16 and x.dim() == 2
            and x.shape[1] % 16 == 0 and 16 <= x.shape[1] <= 1024)
    if gather_dtype is None:
        gather_dtype = getattr(shard, "gather_dtype", None)
        if gather_dtype == "fp8" and not fits:
            gather_dtype = None
    if gather_dtype not in (None, "bf16", "fp8"):
        raise ValueError("scatter_gather: gather_dtype must be None, 'bf16' "
                         f"or 'fp8', got {gather_dtype!r}")
    if gather_dtype == "fp8" and not fits:
        raise ValueError(
            "scatter_gather: gather_dtype='fp8' needs bf16 x with D % 16 == 0 "
            f"and D <= 1024, got {x.dtype} {tuple(x.shape)}")
    extra = ()
    if gather_dtype == "fp8":
        if relu or grad_src_scale is not None:
            raise ValueError("scatter_gather: relu / grad_src_scale do not "
                             "combine with gather_dtype='fp8'")
    else:
        loss = None
        if loss_rows_only and getattr(shard, "bwd_loss_strips", None):
            loss = (shard.bwd_loss_strips, shard.bwd_loss_heavy,
                    shard.loss_keep)
        extra = (relu, grad_src_scale, loss)
    op = _SpMMFp8 if gather_dtype == "fp8" else _SpMM
    return op.apply(
        x, shard.rowptr, shard.colidx, shard.t_rowptr, shard.t_colidx,
        shard.n_local, shard.n_ext, deg_dst, deg_src,
        shard.row_order, shard.t_row_order,
        shard.fwd_strips, shard.bwd_strips,
        getattr(shard, "fwd_strip_heavy", None),
        getattr(shard, "bwd_strip_heavy", None),
        getattr(shard, "strip_heavy_min", 0),
        getattr(shard, "fwd_strip_order", None),
        getattr(shard, "bwd_strip_order", None),
        *extra,
    )


class _SegReduce(torch.autograd.Function):
    """out[v] = max / min over in-neighbors of x[u] (seg_max.hip). arg is
    the winning forward edge per (row, column); the backward is a
    deterministic gather over the transpose CSR that adds dy[v, j] to
    source u where arg[v, j] names the forward edge of the transposed
    edge (u, v) — no atomics. arg is produced and saved only when x needs
    a gradient (or the caller asks for it); t_eperm is a thunk for the
    int32 transposed-edge -> forward-edge map and is called only then."""

    @staticmethod
    def forward(ctx, x, rowptr, colidx, t_rowptr, t_colidx, t_eperm,
                num_rows, num_src, is_min, row_order, t_row_order,
                return_arg):
        need_grad = ctx.needs_input_grad[0]
        x = x.contiguous()
        arg = None
        if _hip(x):
            out = torch.empty(num_rows, x.shape[1], dtype=x.dtype,
                              device=x.device)
            if need_grad or return_arg:
                arg = torch.empty(num_rows, x.shape[1], dtype=torch.int32,
                                  device=x.device)
            _C.seg_max_fwd(out, arg, x, rowptr, colidx, row_order, is_min)
        else:
            out, arg = ref.seg_max(x, rowptr, colidx, num_rows,
                                   "min" if is_min else "max")
        ctx.num_src = num_src
        if need_grad:
            if x.is_cuda:
                ctx.save_for_backward(arg, t_rowptr, t_colidx, t_eperm(),
                                      t_row_order)
            else:
                ctx.save_for_backward(arg, rowptr, colidx)
        if not return_arg:
            arg = torch.empty(0, dtype=torch.int32, device=x.device)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, dy, _darg):
        dy = dy.contiguous()
        if _hip(dy):
            arg, t_rowptr, t_colidx, t_eperm, t_row_order = ctx.saved_tensors
            dx = torch.empty(ctx.num_src, dy.shape[1], dtype=dy.dtype,
                             device=dy.device)
            _C.seg_max_bwd(dx, dy, arg, t_rowptr, t_colidx, t_eperm,
                           t_row_order)
        else:
            arg, rowptr, colidx = ctx.saved_tensors
            dx = ref.seg_max_grad(dy, arg, rowptr, colidx, ctx.num_src)
        return (dx,) + (None,) * 11


def _check_reduce(reduce: str) -> bool:
    if reduce not in ("max", "min"):
        raise ValueError(f"reduce must be 'max' or 'min', got {reduce!r}")
    return reduce == "min"


def seg_reduce_csr(x, rowptr, colidx, t_rowptr, t_colidx, t_eperm, num_rows,
                   num_src, reduce="max", row_order=None, t_row_order=None,
                   return_arg=False):
    """scatter_gather_reduce over an explicit CSR / transpose-CSR pair.
    t_eperm: a callable returning the int32 [E] map from transposed edge
    to forward edge (the stable argsort of colidx)."""
    if x.dim() != 2 or x.shape[0] != num_src:
        # colidx indexes x unchecked on the GPU: a short x reads out of bounds
        raise ValueError(f"x must be [{num_src}, D], got {tuple(x.shape)}")
    out, arg = _SegReduce.apply(
        x, rowptr, colidx, t_rowptr, t_colidx, t_eperm, num_rows, num_src,
        _check_reduce(reduce), row_order, t_row_order, return_arg)
    return (out, arg) if return_arg else out


def scatter_gather_reduce(x, shard, reduce: str = "max",
                          return_arg: bool = False):
    """Neighbor max / min aggregation over the shard's local CSR (the
    reference's declared-but-dead AGGR_MAX / AGGR_MIN).

    x: [n_ext, D] halo-extended features. Returns [n_local, D] in x's
    dtype; every output element is one of the inputs bit for bit. Among
    equal values the first edge in CSR order wins and takes the whole
    gradient; rows without edges give 0 and pass no gradient.
    return_arg=True also returns arg, int32 [n_local, D]: the local CSR
    edge index of each winner (-1 on empty rows). `shard` may be a
    GraphShard or a sampling Block; a Block has no cached edge
    permutation, so its backward map is computed per call."""
    return seg_reduce_csr(
        x, shard.rowptr, shard.colidx, shard.t_rowptr, shard.t_colidx,
        _edge_perm_thunk(shard), shard.n_local, shard.n_ext, reduce,
        shard.row_order, shard.t_row_order, return_arg)


class _SegStats(torch.autograd.Function):
    """out[v] = [mean | std | max | min] over in-neighbors of x[u], all four
    from one gather of each neighbor row (seg_stats.hip). When x needs a
    gradient the forward also saves stats (fp32 [mean | 1/std], so the
    backward never sees the rounded out) and arg (the winning forward edges
    of max and min). The backward is one deterministic gather over the
    transpose CSR — no atomics. t_eperm is a thunk, called only when a
    gradient is needed."""

    @staticmethod
    def forward(ctx, x, rowptr, colidx, t_rowptr, t_colidx, t_eperm,
                num_rows, num_src, eps, row_order, t_row_order):
        need_grad = ctx.needs_input_grad[0]
        x = x.contiguous()
        if _hip(x):
            D = x.shape[1]
            out = torch.empty(num_rows, 4 * D, dtype=x.dtype, device=x.device)
            stats = arg = None
            if need_grad:
                stats = torch.empty(num_rows, 2 * D, dtype=torch.float32,
                                    device=x.device)
                arg = torch.empty(num_rows, 2 * D, dtype=torch.int32,
                                  device=x.device)
            _C.seg_stats_fwd(out, stats, arg, x, rowptr, colidx, row_order,
                             eps)
        else:
            out, stats, arg = ref.seg_stats(x, rowptr, colidx, num_rows, eps)
        ctx.num_src = num_src
        if need_grad:
            if x.is_cuda:
                ctx.save_for_backward(x, stats, arg, rowptr, t_rowptr,
                                      t_colidx, t_eperm(), t_row_order)
            else:
                ctx.save_for_backward(x, stats, arg, rowptr, colidx)
        return out

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        if _hip(dy):
            (x, stats, arg, rowptr, t_rowptr, t_colidx, t_eperm,
             t_row_order) = ctx.saved_tensors
            dx = torch.empty_like(x)
            _C.seg_stats_bwd(dx, dy, x, stats, arg, rowptr, t_rowptr,
                             t_colidx, t_eperm, t_row_order)
        else:
            x, stats, arg, rowptr, colidx = ctx.saved_tensors
            dx = ref.seg_stats_grad(dy, x, stats, arg, rowptr, colidx,
                                    ctx.num_src)
        return (dx,) + (None,) * 10


def seg_stats_csr(x, rowptr, colidx, t_rowptr, t_colidx, t_eperm, num_rows,
                  num_src, eps=1e-5, row_order=None, t_row_order=None):
    """scatter_gather_stats over an explicit CSR / transpose-CSR pair.
    t_eperm: a callable returning the int32 [E] map from transposed edge
    to forward edge (the stable argsort of colidx)."""
    if x.dim() != 2 or x.shape[0] != num_src:
        # colidx indexes x unchecked on the GPU: a short x reads out of bounds
        raise ValueError(f"x must be [{num_src}, D], got {tuple(x.shape)}")
    return _SegStats.apply(x, rowptr, colidx, t_rowptr, t_colidx, t_eperm,
                           num_rows, num_src, float(eps), row_order,
                           t_row_order)


def _edge_perm_thunk(shard):
    """The shard's cached int32 transposed-edge -> forward-edge map; a
    sampling Block has none, so its map is computed per call."""
    cached = getattr(shard, "t_edge_perm32", None)
    if cached is None:
        def cached():
            return torch.argsort(shard.colidx.long(), stable=True).int()
    return cached


def scatter_gather_stats(x, shard, eps: float = 1e-5):
    """The four PNA aggregators over the shard's local CSR in one pass.

    x: [n_ext, D] halo-extended features. Returns [n_local, 4*D] in x's
    dtype, laid out [mean | std | max | min]: std = sqrt(var + eps) with
    the population variance, max / min as scatter_gather_reduce gives them
    (bit for bit an input, first edge wins ties and takes the whole
    gradient). Rows without edges give 0 and pass no gradient. `shard` may
    be a GraphShard or a sampling Block."""
    return seg_stats_csr(
        x, shard.rowptr, shard.colidx, shard.t_rowptr, shard.t_colidx,
        _edge_perm_thunk(shard), shard.n_local, shard.n_ext, eps,
        shard.row_order, shard.t_row_order)


class _SegSoftmax(torch.autograd.Function):
    """out[v, j] = sum_e softmax_e(t * x[u_e, j]) * x[u_e, j] over the
    in-neighbours of v, one softmax per column, out of one gather of each
    neighbour row (seg_softmax.hip). When x or t needs a gradient the
    forward also saves stats, fp32 [lse | out] with the log-sum-exp of the
    scores centred on out (the backward never sees the rounded out). The backward is one deterministic gather over the
    transpose CSR: no edge permutation, no atomics; dt is folded in a fixed
    order and is skipped when t needs no gradient."""

    @staticmethod
    def forward(ctx, x, t, rowptr, colidx, t_rowptr, t_colidx, num_rows,
                num_src, row_order, t_row_order):
        need_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        x = x.contiguous()
        if _hip(x):
            out = torch.empty(num_rows, x.shape[1], dtype=x.dtype,
                              device=x.device)
            stats = None
            if need_grad:
                stats = torch.empty(num_rows, 2 * x.shape[1],
                                    dtype=torch.float32, device=x.device)
            _C.seg_softmax_fwd(out, stats, x, t, rowptr, colidx, row_order)
        else:
            out, stats = ref.seg_softmax(x, t, rowptr, colidx, num_rows)
        ctx.num_src = num_src
        if need_grad:
            if x.is_cuda:
                ctx.save_for_backward(x, stats, t, t_rowptr, t_colidx,
                                      t_row_order)
            else:
                ctx.save_for_backward(x, stats, t, rowptr, colidx)
        return out

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dt = None
        if _hip(dy):
            x, stats, t, t_rowptr, t_colidx, t_row_order = ctx.saved_tensors
            dx = torch.empty_like(x)
            if ctx.needs_input_grad[1]:
                dt = torch.empty_like(t)
            _C.seg_softmax_bwd(dx, dt, dy, x, stats, t, t_rowptr, t_colidx,
                               t_row_order)
        else:
            x, stats, t, rowptr, colidx = ctx.saved_tensors
            dx, dt = ref.seg_softmax_grad(dy, x, stats, t, rowptr, colidx,
                                          ctx.num_src)
            dt = dt.to(t.dtype).view_as(t)
        return (dx, dt) + (None,) * 8


def seg_softmax_csr(x, t, rowptr, colidx, t_rowptr, t_colidx, num_rows,
                    num_src, row_order=None, t_row_order=None):
    """scatter_gather_softmax over an explicit CSR / transpose-CSR pair.
    Every argument is checked here, before any launch."""
    if x.dim() != 2 or x.shape[0] != num_src:
        # colidx indexes x unchecked on the GPU: a short x reads out of bounds
        raise ValueError(f"x must be [{num_src}, D], got {tuple(x.shape)}")
    if x.is_cuda and x.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(
            f"scatter_gather_softmax on GPU takes bf16 or fp32, got {x.dtype}")
    ok = (torch.float32, torch.float64) if x.dtype == torch.float64 \
        else (torch.float32,)
    if not torch.is_tensor(t) or t.dtype not in ok or t.numel() != 1:
        raise ValueError("the temperature must be a fp32 tensor of one "
                         "element (read on the device, never on the host)")
    if t.device != x.device:
        raise ValueError("x and the temperature must live on one device")
    return _SegSoftmax.apply(x, t, rowptr, colidx, t_rowptr, t_colidx,
                             num_rows, num_src, row_order, t_row_order)


def scatter_gather_softmax(x, shard, t):
    """DeeperGCN's softmax aggregation over the shard's local CSR (Li et al.
    2020, PyG's GENConv with aggr="softmax").

    x: [n_ext, D] halo-extended features; t: the temperature, a fp32 tensor
    of one element on x's device (a learnable parameter or a buffer). For
    row v, column j and in-edge e from u_e:
      p_e = softmax_e(t * x[u_e, j]),   out[v, j] = sum_e p_e * x[u_e, j]
    t = 0 is the mean and t -> inf the max. Returns [n_local, D] in x's
    dtype (bf16 or fp32 on GPU; all arithmetic is fp32, one rounding at the
    store). Duplicate edges each count; a row without edges gives 0 and
    passes no gradient; a source without out-edges gets a zero gradient.
    The gradient of t is reduced without atomics in a fixed order:
    bit-reproducible from run to run. `shard` may be a GraphShard or a
    sampling Block."""
    return seg_softmax_csr(
        x, t, shard.rowptr, shard.colidx, shard.t_rowptr, shard.t_colidx,
        shard.n_local, shard.n_ext, shard.row_order, shard.t_row_order)


# ---------------------------------------------------------------------------
# Dot-product graph attention (fused online-softmax kernels)
# ---------------------------------------------------------------------------

class _GraphAttention(torch.autograd.Function):
    """GPU path of graph_attention (graph_attn.hip). The forward saves
    out and a fp32 [n, H] log-sum-exp; the backward is two gather passes
    that recompute p = exp(s - lse): destination-major for delta and dq,
    source-major over the transpose CSR for dkv. No [E] tensor, no
    atomics. need_lse is False when nothing needs a gradient (decided by
    the caller: grad mode is always off in here); the kernel variant
    without the lse store runs then."""

    @staticmethod
    def forward(ctx, q, kv, rowptr, colidx, t_rowptr, t_colidx, heads, scale,
                row_order, t_row_order, need_lse):
        out = torch.empty_like(q)
        lse = None
        if need_lse:
            lse = torch.empty(q.shape[0], heads, dtype=torch.float32,
                              device=q.device)
        _C.graph_attn_fwd(out, lse, q, kv, rowptr, colidx, row_order, heads,
                          scale)
        if need_lse:
            ctx.save_for_backward(q, kv, out, lse, rowptr, colidx, t_rowptr,
                                  t_colidx, row_order, t_row_order)
        ctx.heads, ctx.scale = heads, scale
        return out

    @staticmethod
    def backward(ctx, dy):
        (q, kv, out, lse, rowptr, colidx, t_rowptr, t_colidx, row_order,
         t_row_order) = ctx.saved_tensors
        dy = dy.contiguous()
        dq = torch.empty_like(q)
        delta = torch.empty_like(lse)
        _C.graph_attn_bwd_dst(dq, delta, dy, out, lse, q, kv, rowptr, colidx,
                              row_order, ctx.heads, ctx.scale)
        dkv = None
        if ctx.needs_input_grad[1]:
            dkv = torch.empty_like(kv)
            _C.graph_attn_bwd_src(dkv, q, dy, lse, delta, kv, t_rowptr,
                                  t_colidx, t_row_order, ctx.heads, ctx.scale)
        return (dq, dkv) + (None,) * 9


def graph_attention_csr(q, kv, rowptr, colidx, t_rowptr, t_colidx, num_rows,
                        num_src, heads, scale=None, row_order=None,
                        t_row_order=None):
    """graph_attention over an explicit CSR / transpose-CSR pair. Every
    argument is checked here, before any launch."""
    heads = int(heads)
    if q.dim() != 2 or q.shape[0] != num_rows:
        raise ValueError(f"q must be [{num_rows}, D], got {tuple(q.shape)}")
    D = q.shape[1]
    if heads < 1 or D < heads or D % heads != 0:
        raise ValueError(
            f"feature dim {D} is not a positive multiple of {heads} heads")
    if tuple(kv.shape) != (num_src, 2 * D):
        # colidx indexes kv unchecked on the GPU: a short kv reads out of
        # bounds
        raise ValueError(
            f"kv must be [{num_src}, {2 * D}], got {tuple(kv.shape)}")
    if q.dtype != kv.dtype:
        raise ValueError(
            f"q and kv must share a dtype, got {q.dtype} and {kv.dtype}")
    if q.is_cuda and q.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(
            f"graph_attention on GPU takes bf16 or fp32, got {q.dtype}")
    if scale is None:
        scale = float(D // heads) ** -0.5
    scale = float(scale)
    if not _hip(q):
        return ref.graph_attention(q, kv, rowptr, colidx, num_rows, heads,
                                   scale)
    need_lse = torch.is_grad_enabled() and (q.requires_grad
                                            or kv.requires_grad)
    return _GraphAttention.apply(
        q.contiguous(), kv.contiguous(), rowptr, colidx, t_rowptr, t_colidx,
        heads, scale, row_order, t_row_order, need_lse)


def graph_attention(q, kv, shard, heads: int, scale: Optional[float] = None):
    """Scaled dot-product attention over each node's in-neighbourhood
    (PyG's TransformerConv, the UniMP / graph-transformer family).

    q: [n_local, D], D = heads * dh. kv: [n_ext, 2*D], halo-extended, K
    in columns [0, D) and V in [D, 2D): one projection GEMM and one halo
    exchange serve both. For row v, head h and in-edge e from u_e:
      s_e = scale * <q[v,h,:], K[u_e,h,:]>,  alpha = softmax_e(s),
      out[v,h,:] = sum_e alpha_e * V[u_e,h,:]
    scale defaults to dh ** -0.5. Returns [n_local, D] in q's dtype
    (bf16 or fp32 on GPU; all arithmetic is fp32, one rounding at the
    store). Duplicate edges each count; a row without edges gives 0 and
    passes no gradient; a source without out-edges gets a zero gradient.
    `shard` may be a GraphShard or anything with the same CSR fields."""
    return graph_attention_csr(
        q, kv, shard.rowptr, shard.colidx, shard.t_rowptr, shard.t_colidx,
        shard.n_local, shard.n_ext, heads, scale, shard.row_order,
        shard.t_row_order)


# ---------------------------------------------------------------------------
# GATv2 dynamic attention (fused one-gather kernels)
# ---------------------------------------------------------------------------

class _GATv2Attention(torch.autograd.Function):
    """GPU path of gatv2_attention (gatv2_attn.hip). The forward saves out
    and a fp32 [n, H] log-sum-exp; the backward is two gather passes that
    recompute z, s and p = exp(s - lse): destination-major for delta, dxr
    and datt (an order-fixed slab fold, no atomics), source-major over the
    transpose CSR for dxl, skipped when xl needs no gradient. need_lse is
    False when nothing needs a gradient (decided by the caller: grad mode
    is always off in here); the kernel variant without the lse store runs
    then."""

    @staticmethod
    def forward(ctx, xl, xr, att, rowptr, colidx, t_rowptr, t_colidx, heads,
                slope, row_order, t_row_order, need_lse):
        out = torch.empty_like(xr)
        lse = None
        if need_lse:
            lse = torch.empty(xr.shape[0], heads, dtype=torch.float32,
                              device=xr.device)
        _C.gatv2_attn_fwd(out, lse, xl, xr, att, rowptr, colidx, row_order,
                          heads, slope)
        if need_lse:
            ctx.save_for_backward(xl, xr, att, out, lse, rowptr, colidx,
                                  t_rowptr, t_colidx, row_order, t_row_order)
        ctx.heads, ctx.slope = heads, slope
        return out

    @staticmethod
    def backward(ctx, dy):
        (xl, xr, att, out, lse, rowptr, colidx, t_rowptr, t_colidx, row_order,
         t_row_order) = ctx.saved_tensors
        dy = dy.contiguous()
        dxr = torch.empty_like(xr)
        datt = torch.empty_like(att)
        delta = torch.empty_like(lse)
        _C.gatv2_attn_bwd_dst(dxr, datt, delta, dy, out, lse, xl, xr, att,
                              rowptr, colidx, row_order, ctx.heads, ctx.slope)
        dxl = None
        if ctx.needs_input_grad[0]:
            dxl = torch.empty_like(xl)
            _C.gatv2_attn_bwd_src(dxl, xl, xr, att, dy, lse, delta, t_rowptr,
                                  t_colidx, t_row_order, ctx.heads, ctx.slope)
        return (dxl, dxr, datt) + (None,) * 9


def gatv2_attention_csr(xl, xr, att, rowptr, colidx, t_rowptr, t_colidx,
                        num_rows, num_src, heads, slope: float = 0.2,
                        row_order=None, t_row_order=None):
    """gatv2_attention over an explicit CSR / transpose-CSR pair. Every
    argument is checked here, before any launch."""
    heads = int(heads)
    if xr.dim() != 2 or xr.shape[0] != num_rows:
        raise ValueError(f"xr must be [{num_rows}, D], got {tuple(xr.shape)}")
    D = xr.shape[1]
    if heads < 1 or D < heads or D % heads != 0:
        raise ValueError(
            f"feature dim {D} is not a positive multiple of {heads} heads")
    if tuple(xl.shape) != (num_src, D):
        # colidx indexes xl unchecked on the GPU: a short xl reads out of
        # bounds
        raise ValueError(
            f"xl must be [{num_src}, {D}], got {tuple(xl.shape)}")
    if xl.dtype != xr.dtype:
        raise ValueError(
            f"xl and xr must share a dtype, got {xl.dtype} and {xr.dtype}")
    if xr.is_cuda and xr.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(
            f"gatv2_attention on GPU takes bf16 or fp32, got {xr.dtype}")
    ok = (torch.float32, torch.float64) if xr.dtype == torch.float64 \
        else (torch.float32,)
    if att.dtype not in ok or tuple(att.shape) != (heads, D // heads):
        raise ValueError(
            f"att must be fp32 [{heads}, {D // heads}], got {att.dtype} "
            f"{tuple(att.shape)}")
    if att.device != xr.device or xl.device != xr.device:
        raise ValueError("xl, xr and att must live on one device")
    slope = float(slope)
    if not _hip(xr):
        return ref.gatv2_attention(xl, xr, att, rowptr, colidx, num_rows,
                                   heads, slope)
    need_lse = torch.is_grad_enabled() and (
        xl.requires_grad or xr.requires_grad or att.requires_grad)
    return _GATv2Attention.apply(
        xl.contiguous(), xr.contiguous(), att.contiguous(), rowptr, colidx,
        t_rowptr, t_colidx, heads, slope, row_order, t_row_order, need_lse)


def gatv2_attention(xl, xr, att, shard, heads: int, slope: float = 0.2):
    """GATv2 dynamic attention over each node's in-neighbourhood (Brody et
    al. 2022, PyG's GATv2Conv).

    xl: [n_ext, D], halo-extended, D = heads * dh: the source projection,
    which is both the score row and the value row. xr: [n_local, D], the
    destination projection. att: fp32 [heads, dh], used as it is (fp64 is
    accepted next to fp64 inputs on CPU, for gradcheck). For row v, head h
    and in-edge e from u_e:
      s_e = sum_j att[h,j] * lrelu(xl[u_e,h,j] + xr[v,h,j]),
      alpha = softmax_e(s),  out[v,h,:] = sum_e alpha_e * xl[u_e,h,:]
    Returns [n_local, D] in xr's dtype (bf16 or fp32 on GPU; all arithmetic
    is fp32, one rounding at the store). Duplicate edges each count; a row
    without edges gives 0 and passes no gradient; a source without
    out-edges gets a zero gradient. The gradient of att is reduced without
    atomics in a fixed order: bit-reproducible from run to run.
    `shard` may be a GraphShard or anything with the same CSR fields."""
    return gatv2_attention_csr(
        xl, xr, att, shard.rowptr, shard.colidx, shard.t_rowptr,
        shard.t_colidx, shard.n_local, shard.n_ext, heads, slope,
        shard.row_order, shard.t_row_order)


# ---------------------------------------------------------------------------
# Edge-gated aggregation (fused per-column sigmoid-gate kernels)
# ---------------------------------------------------------------------------

class _GatedAggregate(torch.autograd.Function):
    """GPU path of gated_aggregate (gated_agg.hip). In the mean form the
    forward saves stats, fp32 [den | out32]: the backward never sees the
    rounded out. The sum form saves nothing. The backward is two gather
    passes that recompute the gates: destination-major for dq, source-major
    over the transpose CSR for dkv, each skipped when its input needs no
    gradient. No [E, D] tensor, no atomics. need_stats is False when nothing
    needs a gradient (decided by the caller: grad mode is always off in
    here); the kernel variant without the state stores runs then."""

    @staticmethod
    def forward(ctx, q, kv, rowptr, colidx, t_rowptr, t_colidx, normalize,
                eps, row_order, t_row_order, need_stats):
        out = torch.empty_like(q)
        stats = None
        if need_stats and normalize:
            stats = torch.empty(q.shape[0], 2 * q.shape[1],
                                dtype=torch.float32, device=q.device)
        _C.gated_agg_fwd(out, stats, q, kv, rowptr, colidx, row_order,
                         normalize, eps)
        if need_stats:
            # stats is None in the sum form; save_for_backward takes it
            ctx.save_for_backward(q, kv, stats, rowptr, colidx, t_rowptr,
                                  t_colidx, row_order, t_row_order)
        ctx.normalize = normalize
        return out

    @staticmethod
    def backward(ctx, dy):
        (q, kv, stats, rowptr, colidx, t_rowptr, t_colidx, row_order,
         t_row_order) = ctx.saved_tensors
        dy = dy.contiguous()
        dq = dkv = None
        if ctx.needs_input_grad[0]:
            dq = torch.empty_like(q)
            _C.gated_agg_bwd_dst(dq, dy, stats, q, kv, rowptr, colidx,
                                 row_order, ctx.normalize)
        if ctx.needs_input_grad[1]:
            dkv = torch.empty_like(kv)
            _C.gated_agg_bwd_src(dkv, dy, stats, q, kv, t_rowptr, t_colidx,
                                 t_row_order, ctx.normalize)
        return (dq, dkv) + (None,) * 9


def gated_aggregate_csr(q, kv, rowptr, colidx, t_rowptr, t_colidx, num_rows,
                        num_src, normalize: bool = True, eps: float = 1e-6,
                        row_order=None, t_row_order=None):
    """gated_aggregate over an explicit CSR / transpose-CSR pair. Every
    argument is checked here, before any launch."""
    if q.dim() != 2 or q.shape[0] != num_rows:
        raise ValueError(f"q must be [{num_rows}, D], got {tuple(q.shape)}")
    D = q.shape[1]
    if tuple(kv.shape) != (num_src, 2 * D):
        # colidx indexes kv unchecked on the GPU: a short kv reads out of
        # bounds
        raise ValueError(
            f"kv must be [{num_src}, {2 * D}], got {tuple(kv.shape)}")
    if q.dtype != kv.dtype:
        raise ValueError(
            f"q and kv must share a dtype, got {q.dtype} and {kv.dtype}")
    if q.device != kv.device:
        raise ValueError("q and kv must live on one device")
    if q.is_cuda and q.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(
            f"gated_aggregate on GPU takes bf16 or fp32, got {q.dtype}")
    normalize, eps = bool(normalize), float(eps)
    if normalize and not eps > 0.0:
        # a row whose gates all underflow has a zero gate sum
        raise ValueError(f"the mean form needs eps > 0, got {eps}")
    if int(colidx.numel()) >= 2 ** 31:
        raise ValueError("2^31 or more edges do not fit the int32 edge index")
    if not _hip(q):
        return ref.gated_aggregate(q, kv, rowptr, colidx, num_rows, normalize,
                                   eps)
    need_stats = torch.is_grad_enabled() and (q.requires_grad
                                              or kv.requires_grad)
    return _GatedAggregate.apply(
        q.contiguous(), kv.contiguous(), rowptr, colidx, t_rowptr, t_colidx,
        normalize, eps, row_order, t_row_order, need_stats)


def gated_aggregate(q, kv, shard, normalize: bool = True, eps: float = 1e-6):
    """Edge-gated aggregation over each node's in-neighbourhood (Bresson &
    Laurent's residual gated graph ConvNet, PyG's ResGatedGraphConv).

    q: [n_local, D], the destination projection. kv: [n_ext, 2*D],
    halo-extended, the gate's source half k in columns [0, D) and the
    values in [D, 2D): one projection GEMM and one halo exchange serve
    both. For row v, column j and in-edge e from u_e:
      eta[e, j] = sigmoid(q[v, j] + k[u_e, j])
      out[v, j] = sum_e eta[e, j] * val[u_e, j]
    and in the mean form (normalize, the default) that sum divided by
    sum_e eta[e, j] + eps: a plain gated sum grows with the degree. Returns
    [n_local, D] in q's dtype (bf16 or fp32 on GPU; all arithmetic is fp32,
    one rounding at the store). The gate stays finite at any q + k.
    Duplicate edges each count; a row without edges gives 0 and passes no
    gradient; a source without out-edges gets a zero gradient. `shard` may
    be a GraphShard, a sampling Block or anything with the same CSR
    fields."""
    return gated_aggregate_csr(
        q, kv, shard.rowptr, shard.colidx, shard.t_rowptr, shard.t_colidx,
        shard.n_local, shard.n_ext, normalize, eps, shard.row_order,
        shard.t_row_order)


# ---------------------------------------------------------------------------
# InDegreeNorm
# ---------------------------------------------------------------------------

class _DegScale(torch.autograd.Function):
    """out = x * scale_row (rowwise). Self-adjoint: backward applies the
    same scaling to the gradient (reference `graphnorm_kernel.cu:126-136`)."""

    @staticmethod
    def forward(ctx, x, scale):
        ctx.save_for_backward(scale)
        if _hip(x):
            out = torch.empty_like(x)
            _C.rowscale(out, x, scale)
        else:
            out = x * scale.unsqueeze(1).to(x.dtype)
        return out

    @staticmethod
    def backward(ctx, dy):
        (scale,) = ctx.saved_tensors
        dy = dy.contiguous()
        if _hip(dy):
            dx = torch.empty_like(dy)
            _C.rowscale(dx, dy, scale)
        else:
            dx = dy * scale.unsqueeze(1).to(dy.dtype)
        return dx, None


def indegree_norm(x, shard):
    """out[v] = x[v] / sqrt(indeg(v)) on local rows (reference graphnorm op)."""
    return _DegScale.apply(x, shard.rsqrt_deg_local)


def degree_scale(x, scale):
    """Generic rowwise scale (used by GraphSAGE mean aggregation: 1/deg)."""
    return _DegScale.apply(x, scale)


# ---------------------------------------------------------------------------
# LayerNorm (+ fused ReLU), per node
# ---------------------------------------------------------------------------

LAYER_NORM_MAX_D = 1024  # the kernel holds a whole row in registers


class _LayerNorm(torch.autograd.Function):
    """y = act((x - mean) * rstd * gamma + beta) per row (layer_norm.hip).
    Saves x and the two fp32 [N] row statistics; the backward recomputes
    x-hat and the relu mask from them, so no [N, D] intermediate is kept.
    need_stats is False when nothing needs a gradient (decided by the
    caller: grad mode is always off in here); the kernel variant without
    the statistics stores runs then. dgamma / dbeta come from an
    order-fixed slab fold (no atomics, bit-reproducible)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, relu, need_stats):
        need = need_stats
        x = x.contiguous()
        if _hip(x):
            y = torch.empty_like(x)
            mean = rstd = None
            if need:
                mean = torch.empty(x.shape[0], dtype=torch.float32,
                                   device=x.device)
                rstd = torch.empty_like(mean)
            _C.layer_norm_fwd(y, mean, rstd, x, gamma, beta, eps, relu)
        else:
            y, mean, rstd = ref.layer_norm(x, gamma, beta, eps, relu)
        if need:
            ctx.save_for_backward(x, mean, rstd, gamma, beta)
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, gamma, beta = ctx.saved_tensors
        dy = dy.contiguous()
        if _hip(dy):
            dx = torch.empty_like(x)
            dgamma = torch.empty_like(gamma)
            dbeta = torch.empty_like(beta)
            _C.layer_norm_bwd(dx, dgamma, dbeta, dy, x, mean, rstd, gamma,
                              beta, ctx.relu)
        else:
            dx, dgamma, dbeta = ref.layer_norm_grad(
                dy, x, mean, rstd, gamma, beta, ctx.relu)
            dgamma = dgamma.to(gamma.dtype)
            dbeta = dbeta.to(beta.dtype)
        return dx, dgamma, dbeta, None, None, None


def layer_norm(x, gamma, beta, eps: float = 1e-5,
               activation: Optional[str] = None):
    """Per-row LayerNorm over the feature dim with an optional fused ReLU.

    x: [N, D], D <= 1024; bf16 (D % 8 == 0) or fp32 on GPU. gamma, beta:
    fp32 [D] masters, used as they are (fp64 is accepted next to an fp64
    x on CPU, for gradcheck). Row-local, so exact at any world size, on
    sampled blocks and under recompute. Every argument is checked here,
    before any launch."""
    if activation not in (None, "relu"):
        raise ValueError(
            f"activation must be None or 'relu', got {activation!r}")
    if x.dim() != 2:
        raise ValueError(f"x must be [N, D], got {tuple(x.shape)}")
    D = x.shape[1]
    if D < 1 or D > LAYER_NORM_MAX_D:
        raise ValueError(
            f"layer_norm supports 1 <= D <= {LAYER_NORM_MAX_D}, got D = {D}")
    if x.is_cuda and x.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"layer_norm on GPU takes bf16 or fp32, got {x.dtype}")
    if x.dtype == torch.bfloat16 and D % 8 != 0:
        raise ValueError(
            f"bf16 rows must be a multiple of 8 wide (16 B), got D = {D}")
    ok = (torch.float32, torch.float64) if x.dtype == torch.float64 \
        else (torch.float32,)
    for name, p in (("gamma", gamma), ("beta", beta)):
        if p.dtype not in ok or tuple(p.shape) != (D,):
            raise ValueError(
                f"{name} must be fp32 [{D}], got {p.dtype} {tuple(p.shape)}")
    need_stats = torch.is_grad_enabled() and (
        x.requires_grad or gamma.requires_grad or beta.requires_grad)
    return _LayerNorm.apply(x, gamma.contiguous(), beta.contiguous(),
                            float(eps), activation == "relu", need_stats)


# ---------------------------------------------------------------------------
# BatchNorm (+ fused ReLU), over the nodes of all shards
# ---------------------------------------------------------------------------

def _in_backward_pass() -> bool:
    """True inside a checkpoint's re-forward (it runs in the backward pass);
    the running statistics were already advanced by the first forward."""
    return torch._C._current_graph_task_id() != -1


class _BatchNorm(torch.autograd.Function):
    """y = act(((x - mean_j) * rstd_j) * gamma_j + beta_j) with column
    statistics over the rows of every rank (batch_norm.hip). Saves x and the
    fp32 [D] mean and rstd; the backward recomputes x-hat and the relu mask,
    so no [N, D] intermediate is kept. The cross-rank merges are all_reduce
    only (capturable). dgamma / dbeta returned to autograd are this rank's
    sums: the trainer's gradient all-reduce adds them over ranks."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training,
                momentum, eps, relu, group, world_size, n, update):
        x = x.contiguous()
        hip = _hip(x)
        if training:
            if hip:
                mean = torch.empty(x.shape[1], dtype=torch.float32,
                                   device=x.device)
                m2 = torch.empty_like(mean)
                _C.batch_norm_stats(mean, m2, x)
            else:
                mean, m2 = ref.batch_norm_stats(x)
            if world_size > 1:
                import torch.distributed as dist
                n_r = x.shape[0]
                mean_g = mean * n_r
                dist.all_reduce(mean_g, group=group)
                mean_g /= n
                m2 = m2 + n_r * (mean - mean_g) ** 2
                dist.all_reduce(m2, group=group)
                mean = mean_g
            rm, rv = (running_mean, running_var) if update else (None, None)
            if hip:
                rstd = torch.empty_like(mean)
                _C.batch_norm_finalize(rstd, mean, m2, rm, rv, n, momentum,
                                       eps)
            else:
                rstd = ref.batch_norm_finalize(mean, m2, n, eps, rm, rv,
                                               momentum)
        else:
            mean = running_mean.to(gamma.dtype)
            rstd = 1.0 / torch.sqrt(running_var.to(gamma.dtype) + eps)
        if hip:
            y = torch.empty_like(x)
            _C.batch_norm_apply(y, x, mean, rstd, gamma, beta, relu)
        else:
            y = ref.batch_norm_apply(x, mean, rstd, gamma, beta, relu)
        ctx.save_for_backward(x, mean, rstd, gamma, beta)
        ctx.cfg = (training, relu, group, world_size, n)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, gamma, beta = ctx.saved_tensors
        training, relu, group, world_size, n = ctx.cfg
        dy = dy.contiguous()
        hip = _hip(dy)
        if hip:
            sums = torch.empty(2, x.shape[1], dtype=torch.float32,
                               device=x.device)
            _C.batch_norm_bwd_reduce(sums[0], sums[1], dy, x, mean, rstd,
                                     gamma, beta, relu)
        else:
            sums = torch.stack(ref.batch_norm_bwd_reduce(
                dy, x, mean, rstd, gamma, beta, relu))
        dgamma, dbeta = sums[0].to(gamma.dtype), sums[1].to(beta.dtype)
        if not training:
            # fixed statistics: dx = gamma * rstd * g, the formula at S = 0
            tot, n = torch.zeros_like(sums), max(x.shape[0], 1)
        elif world_size > 1:
            import torch.distributed as dist
            tot = sums.clone()  # the returned gradients stay local
            dist.all_reduce(tot, group=group)
        else:
            tot = sums
        if hip:
            dx = torch.empty_like(x)
            _C.batch_norm_bwd_dx(dx, dy, x, mean, rstd, gamma, beta, tot[1],
                                 tot[0], n, relu)
        else:
            dx = ref.batch_norm_bwd_dx(dy, x, mean, rstd, gamma, beta,
                                       tot[1], tot[0], n, relu)
        return (dx, dgamma, dbeta) + (None,) * 10


def batch_norm(x, gamma, beta, running_mean=None, running_var=None,
               training: bool = True, momentum: float = 0.1,
               eps: float = 1e-5, activation: Optional[str] = None,
               group=None, world_size: int = 1,
               n_total: Optional[int] = None):
    """BatchNorm over the rows (nodes) of [N, D] with an optional fused ReLU.

    x: this rank's rows; bf16 (D % 8 == 0) or fp32 on GPU, any D. gamma,
    beta: fp32 [D] masters (fp64 next to an fp64 x on CPU, for gradcheck).
    running_mean / running_var: fp32 [D] buffers or None. In training the
    statistics are those of the batch: at world_size > 1 of the n_total rows
    of all ranks, merged with all_reduce over `group`, and every rank must
    call (a rank with no rows too). The running buffers advance in place,
    once per step: a checkpoint's re-forward inside the backward pass leaves
    them alone. In eval the running buffers normalise. Every argument is
    checked here, before any launch."""
    if activation not in (None, "relu"):
        raise ValueError(
            f"activation must be None or 'relu', got {activation!r}")
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError(f"x must be [N, D >= 1], got {tuple(x.shape)}")
    D = x.shape[1]
    if x.is_cuda and x.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"batch_norm on GPU takes bf16 or fp32, got {x.dtype}")
    if x.dtype == torch.bfloat16 and D % 8 != 0:
        raise ValueError(
            f"bf16 rows must be a multiple of 8 wide (16 B), got D = {D}")
    ok = (torch.float32, torch.float64) if x.dtype == torch.float64 \
        else (torch.float32,)
    for name, p in (("gamma", gamma), ("beta", beta)):
        if p.dtype not in ok or tuple(p.shape) != (D,):
            raise ValueError(
                f"{name} must be fp32 [{D}], got {p.dtype} {tuple(p.shape)}")
    if (running_mean is None) != (running_var is None):
        raise ValueError("pass both running buffers, or neither")
    for name, p in (("running_mean", running_mean),
                    ("running_var", running_var)):
        if p is not None and (p.dtype != torch.float32
                              or tuple(p.shape) != (D,)
                              or not p.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous fp32 [{D}] "
                             f"buffer, got {p.dtype} {tuple(p.shape)}")
    if not training and running_mean is None:
        raise ValueError("eval mode normalises with the running buffers")
    if world_size > 1 and n_total is None:
        raise ValueError("world_size > 1 needs n_total, the global row count")
    n = x.shape[0] if n_total is None or world_size == 1 else int(n_total)
    if not 0 < momentum <= 1 or eps <= 0:
        raise ValueError(f"need 0 < momentum <= 1 and eps > 0, got "
                         f"{momentum}, {eps}")
    if training and n < 1:
        raise ValueError("training-mode batch_norm needs at least one row")
    update = training and running_mean is not None \
        and not _in_backward_pass()
    return _BatchNorm.apply(x, gamma.contiguous(), beta.contiguous(),
                            running_mean, running_var, bool(training),
                            float(momentum), float(eps),
                            activation == "relu", group, int(world_size), n,
                            update)


# ---------------------------------------------------------------------------
# Linear (hand-written MFMA GEMM on GPU)
# ---------------------------------------------------------------------------

class _Linear(torch.autograd.Function):
    """y = x @ w (+ fused ReLU). w is an fp32 master [in_dim, out_dim];
    on GPU x is bf16 and w is cast per call (w is tiny: <1 MB).

    Backward: dw = x^T dy (fp32 accumulate, split-K), dx = dy @ w^T.
    Reference: `linear_kernel.cu:20-127` (fwd+fused relu), `:130-245` (bwd).
    """

    @staticmethod
    def forward(ctx, x, w, act, row_scale, grad_prescaled=False):
        # grad_prescaled: dy arrives with row_scale already applied (the
        # consumer's backward stored it so: scatter_gather grad_src_scale)
        ctx.grad_prescaled = grad_prescaled
        if _hip(x):
            # gemm_rr takes B pre-transposed: Bt = w^T [out,in]
            wt, wc = _cast_weight(w, x.dtype)
            ctx.wc = wc
            y = torch.empty(x.shape[0], w.shape[1], dtype=x.dtype, device=x.device)
            _C.gemm_rr(y, x, wt, act == "relu", row_scale)
            if act == "sigmoid":
                _C.sigmoid_fwd(y, y)
        else:
            y = ref.linear(x, w)
            if row_scale is not None:
                y = y * row_scale.unsqueeze(1).to(y.dtype)
            if act == "relu":
                y = ref.relu(y)
            elif act == "sigmoid":
                y = ref.sigmoid(y)
        ctx.save_for_backward(x, w, y if act else None, row_scale)
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y, row_scale = ctx.saved_tensors
        act = ctx.act
        dy = dy.contiguous()
        if _hip(dy):
            if act == "relu":
                dym = torch.empty_like(dy)
                _C.relu_bwd(dym, dy, y)
                dy = dym
            elif act == "sigmoid":
                dym = torch.empty_like(dy)
                _C.sigmoid_bwd(dym, dy, y)
                dy = dym
            if row_scale is not None and not ctx.grad_prescaled:
                dym = torch.empty_like(dy)
                _C.rowscale(dym, dy, row_scale)
                dy = dym
            gbuf = w.grad if _async_dw() else None
            if (gbuf is not None and gbuf.dtype == torch.float32
                    and gbuf.is_contiguous() and gbuf.is_cuda):
                # accumulate straight into .grad on the side stream
                # (gemm_atb is C += ordered split-K sum); return None so
                # autograd does not accumulate a second copy
                from .. import streamcheck
                s = _dw_stream()
                ready = torch.cuda.Event()
                ready.record()  # x/dy produced on the current stream
                s.wait_event(ready)
                with torch.cuda.stream(s):
                    _C.gemm_atb(gbuf, x, dy)
                done = torch.cuda.Event()
                done.record(s)
                streamcheck.producer(done, "dw-gemm")
                _DW_PENDING.append((done, (x, dy)))
                dw = None
            else:
                dw = torch.zeros_like(w)  # fp32 [in, out]
                _C.gemm_atb(dw, x, dy)
            dx = None
            if ctx.needs_input_grad[0]:  # layer-1 inputs carry no grad
                # dx = dy @ w^T: gemm_rr's Bt = (w^T)^T = w [in,out]
                dx = torch.empty_like(x)
                _C.gemm_rr(dx, dy, ctx.wc, False)
        else:
            if act == "relu":
                dy = ref.relu_grad(dy, y)
            elif act == "sigmoid":
                dy = ref.sigmoid_grad(dy, y)
            if row_scale is not None and not ctx.grad_prescaled:
                dy = dy * row_scale.unsqueeze(1).to(dy.dtype)
            dw = (x.to(torch.float32).t() @ dy.to(torch.float32))
            dx = (dy @ w.t().to(dy.dtype)) if ctx.needs_input_grad[0] else None
        return dx, dw, None, None, None


def linear(x, w, activation: Optional[str] = None, row_scale=None,
           grad_prescaled: bool = False):
    """y = act((x @ w) * row_scale). row_scale rides the GEMM epilogue
    (used for the GCN source-degree pre-normalization).
    grad_prescaled=True: the gradient that comes back for y already carries
    row_scale (scatter_gather(grad_src_scale=row_scale) is y's only
    consumer), so the backward does not apply it again. The forward is the
    same either way."""
    return _Linear.apply(x, w, activation, row_scale, grad_prescaled)


# ---------------------------------------------------------------------------
# Standalone activations (reference activation op)
# ---------------------------------------------------------------------------

class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kind):
        if _hip(x):
            y = torch.empty_like(x)
            getattr(_C, f"{kind}_fwd")(y, x)
        else:
            y = ref.relu(x) if kind == "relu" else ref.sigmoid(x)
        ctx.save_for_backward(y)
        ctx.kind = kind
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        if _hip(dy):
            dx = torch.empty_like(dy)
            getattr(_C, f"{ctx.kind}_bwd")(dx, dy, y)
        else:
            dx = ref.relu_grad(dy, y) if ctx.kind == "relu" else ref.sigmoid_grad(dy, y)
        return dx, None


def relu(x):
    return _Act.apply(x, "relu")


def sigmoid(x):
    return _Act.apply(x, "sigmoid")


# ---------------------------------------------------------------------------
# Element (add / mul) — reference element op; autograd-composable
# ---------------------------------------------------------------------------

class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        if _hip(a):
            out = torch.empty_like(a)
            _C.ewise_add(out, a, b)
            return out
        return a + b

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


class _Mul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        if _hip(a):
            out = torch.empty_like(a)
            _C.ewise_mul(out, a, b)
            return out
        return a * b

    @staticmethod
    def backward(ctx, dy):
        a, b = ctx.saved_tensors
        dy = dy.contiguous()
        if _hip(dy):
            da = torch.empty_like(a)
            db = torch.empty_like(b)
            _C.ewise_mul(da, dy, b)
            _C.ewise_mul(db, dy, a)
            return da, db
        return dy * b, dy * a


def add(a, b):
    return _Add.apply(a, b)


def mul(a, b):
    return _Mul.apply(a, b)


# ---------------------------------------------------------------------------
# Dropout (Philox counter-based; mask regenerated in backward — no mask
# tensor is ever materialized on GPU)
# ---------------------------------------------------------------------------

_DROPOUT_STATE = {"seed": 1, "offset": 0, "counter": None, "epoch": 0}
_WEIGHT_VERSION = [0]


def bump_weight_version() -> None:
    """Called by the optimizer after a step: invalidates cached weight
    casts (the per-call w -> bf16 (+transpose) casts are reused within a
    step; disabled under hipGraph capture where the cast kernels must be
    part of the replayed graph)."""
    _WEIGHT_VERSION[0] += 1


def _cast_weight(w, dtype):
    if _DROPOUT_STATE["counter"] is not None:  # capture mode: no caching
        wc = w.contiguous().to(dtype)
        return wc.t().contiguous(), wc
    cache = getattr(w, "_roc_cast", None)
    ver = _WEIGHT_VERSION[0]
    if cache is not None and cache[0] == ver and cache[2].dtype == dtype:
        return cache[1], cache[2]
    wc = w.contiguous().to(dtype)
    wt = wc.t().contiguous()
    w._roc_cast = (ver, wt, wc)
    return wt, wc


def set_dropout_seed(seed: int) -> None:
    _DROPOUT_STATE["seed"] = int(seed)
    _DROPOUT_STATE["offset"] = 0
    _DROPOUT_STATE["epoch"] = 0


def set_dropout_counter(counter) -> None:
    """Device int64[1] epoch counter: makes dropout hipGraph-replayable
    (offset = counter * 65536 + per-epoch call index)."""
    _DROPOUT_STATE["counter"] = counter
    _DROPOUT_STATE["offset"] = 0


def reset_dropout_offset() -> None:
    _DROPOUT_STATE["offset"] = 0


def next_dropout_epoch() -> None:
    """Advance the per-epoch Philox base for call_id-addressed dropout
    (eager path; the hipGraph path gets its epoch from the device
    counter instead). Masks then vary per epoch while staying exactly
    reproducible WITHIN the epoch — the property activation recompute
    needs."""
    _DROPOUT_STATE["epoch"] += 1


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, call_id=None):
        seed = _DROPOUT_STATE["seed"]
        counter = _DROPOUT_STATE["counter"]
        if call_id is not None:
            # stable per-epoch offset: a checkpointed layer re-running its
            # forward during backward regenerates the IDENTICAL mask.
            # Epoch variation: device counter (graph mode) or host epoch.
            offset = int(call_id)
            if counter is None:
                offset += _DROPOUT_STATE["epoch"] * 65536
        else:
            offset = _DROPOUT_STATE["offset"]
            _DROPOUT_STATE["offset"] += 1
        ctx.params = (p, seed, offset, counter)
        if _hip(x):
            y = torch.empty_like(x)
            _C.dropout_fwd(y, x, p, seed, offset, counter)
            return y
        mask = ref.dropout_mask(x.shape, p, seed, offset, x.device)
        ctx.save_for_backward(mask)
        return x * mask.to(x.dtype) / (1.0 - p)

    @staticmethod
    def backward(ctx, dy):
        p, seed, offset, counter = ctx.params
        dy = dy.contiguous()
        if _hip(dy):
            dx = torch.empty_like(dy)
            _C.dropout_fwd(dx, dy, p, seed, offset, counter)  # same stream
            return dx, None, None
        (mask,) = ctx.saved_tensors
        return dy * mask.to(dy.dtype) / (1.0 - p), None, None


def dropout(x, p: float, training: bool, call_id=None):
    """Train: mask+scale; infer: identity (reference `dropout_kernel.cu:159-180`).

    ``call_id``: stable per-epoch Philox offset (= the model's layer
    index). Required under activation recompute; numerically identical
    to the global running offset for the shipped models (one dropout
    per layer, called in layer order)."""
    if not training or p <= 0.0:
        return x
    return _Dropout.apply(x, p, call_id)


# ---------------------------------------------------------------------------
# SoftmaxCrossEntropy (fused loss + grad + metrics)
# ---------------------------------------------------------------------------

class _SoftmaxCE(torch.autograd.Function):
    """Returns (loss, metrics[8]) where metrics =
    [roc_loss_sum, ce_loss_sum, train_correct, train_total,
     val_correct, val_total, test_correct, test_total] (float32, on device).
    loss = ce_loss_sum (differentiable driver for .backward()).
    Gradient: (softmax - onehot) * (mask == Train) * grad_scale
    (reference `softmax_kernel.cu:19-79`).
    """

    @staticmethod
    def forward(ctx, logits, labels, mask, grad_scale, num_classes):
        if _hip(logits):
            dl = torch.empty_like(logits)
            metrics = torch.zeros(8, dtype=torch.float32, device=logits.device)
            _C.softmax_ce(dl, metrics, logits, labels, mask, grad_scale,
                          num_classes or -1)
            loss = metrics[1].clone()
        else:
            dl, md = ref.softmax_cross_entropy(logits, labels, mask,
                                               grad_scale, num_classes)
            metrics = torch.tensor(
                [md["roc_loss"], md["ce_loss"] * max(md["train_total"], 1),
                 md["train_correct"], md["train_total"],
                 md["val_correct"], md["val_total"],
                 md["test_correct"], md["test_total"]],
                dtype=torch.float32)
            # differentiable loss keeps the LOGITS dtype (an fp32 round-trip
            # through the metrics container breaks fp64 gradcheck)
            loss = torch.tensor(md["ce_loss"] * max(md["train_total"], 1),
                                dtype=logits.dtype)
        ctx.save_for_backward(dl)
        ctx.mark_non_differentiable(metrics)
        return loss, metrics

    @staticmethod
    def backward(ctx, dloss, _dmetrics):
        (dl,) = ctx.saved_tensors
        return dl * dloss, None, None, None, None


def softmax_cross_entropy(logits, labels, mask, grad_scale: float = 1.0,
                          num_classes: Optional[int] = None):
    """num_classes < logits width runs softmax over the first num_classes
    columns only (class-dim padding for 16-B-aligned rows)."""
    return _SoftmaxCE.apply(logits, labels, mask, grad_scale, num_classes)


def decode_metrics(metrics: torch.Tensor) -> dict:
    m = metrics.cpu().tolist()
    tt = max(m[3], 1.0)
    return {
        "roc_loss": m[0],
        "ce_loss": m[1] / tt,
        "train_acc": m[2] / tt,
        "val_acc": m[4] / max(m[5], 1.0),
        "test_acc": m[6] / max(m[7], 1.0),
        "train_total": int(m[3]),
        "val_total": int(m[5]),
        "test_total": int(m[7]),
    }


# ---------------------------------------------------------------------------
# Input-row gather of the sampled tier (not autograd — inputs need no grad)
# ---------------------------------------------------------------------------

def gather_rows_cast(feats, ids, out_dtype=None):
    """out[j, :] = feats[ids[j], :] in out_dtype (default: feats' own):
    fp32 -> fp32 / bf16 or bf16 -> bf16, cast in the store (sample.hip).
    One pass over HBM-resident features instead of index, copy and cast."""
    out_dtype = feats.dtype if out_dtype is None else out_dtype
    if _hip(feats):
        out = torch.empty((ids.numel(), feats.shape[1]), dtype=out_dtype,
                          device=feats.device)
        _C.gather_rows_cast(out, feats, ids)
        return out
    return feats[ids].to(out_dtype)


# ---------------------------------------------------------------------------
# Adam (not autograd — called by the optimizer)
# ---------------------------------------------------------------------------

def adam_step(w, g, m, v, alpha_t, beta1, beta2, eps, weight_decay,
              step=None, decay_rate=1.0, decay_steps=100):
    """step (device int64[1]) switches to the hipGraph-replayable mode:
    alpha_t is then the BASE lr and the bias-corrected decayed step size
    is derived on device from the counter."""
    if _hip(w):
        _C.adam_step(w, g, m, v, alpha_t, beta1, beta2, eps, weight_decay,
                     step, decay_rate, decay_steps)
    else:
        ref.adam_step(w, g, m, v, alpha_t, beta1, beta2, eps, weight_decay)
