"""batch_norm.hip on the GPU against the fp64 formulas, the shifted-sum
rule, exact zero variance, bit reproducibility, norm="sync_batch" through a
GCN (GPU against CPU, hipGraph capture against eager) and argument errors."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from roc_amd import (synthetic_dataset, build_shard, build_model,
                     AdamOptimizer, Trainer)
from roc_amd.models.norm import running_stats
from roc_amd.ops import functional as F

DEV = "cuda:0"
EPS, MOM = 1e-5, 0.1

# Worst error of the SAME formulas evaluated with torch in fp32 on the CPU
# (two-pass centred variance; _formulas(case, torch.float32)) against their
# fp64 evaluation, over every case of CASES x relu, as max |err| / max |want|
# per output. The kernels regroup the adds but add no rounding step of their
# own, so they are allowed twice the figure; a bf16 output adds one bf16 ulp
# (2^-7 of the element) for its single rounding at the store.
FP32_FIGURE = {
    "mean": 1.79e-7, "rstd": 1.42e-7, "running_mean": 9.84e-8,
    "running_var": 1.10e-7, "y": 1.74e-7, "dx": 1.21e-7,
    "dgamma": 8.44e-7, "dbeta": 3.45e-7,
}
# the same figures for x = 100 + 0.25 randn, N = 40001, D = 64 (the raw
# sum x^2 - (sum x)^2 / n form, in fp32, is off by 2.7e-2 in rstd there)
SHIFT_FIGURE = {"mean": 1.87e-7, "rstd": 1.79e-7}

CASES = [(n, 8, dt) for n in (1, 3, 1000, 40001)
         for dt in (torch.float32, torch.bfloat16)] + \
        [(3001, d, torch.float32) for d in (1, 5, 64, 260)] + \
        [(3001, d, torch.bfloat16) for d in (8, 72, 256, 520)]


def _case(N, D, dtype):
    gen = torch.Generator().manual_seed(N * 1000 + D)
    x = torch.randn(N, D, generator=gen) * 1.5 + 0.5
    dy = torch.randn(N, D, generator=gen)
    gamma = torch.randn(D, generator=gen) + 1.5
    beta = torch.randn(D, generator=gen) * 0.3
    rm = torch.randn(D, generator=gen)
    rv = torch.rand(D, generator=gen) + 0.5
    return dict(x=x.to(dtype), dy=dy.to(dtype), gamma=gamma, beta=beta,
                rm=rm, rv=rv)


def _formulas(case, ct, relu, stats=None):
    """Every output in compute dtype ct. The backward takes its mean and
    rstd (fp32) from `stats` when given, and its relu mask from the fp32
    evaluation of x-hat*gamma+beta on them: the kernels round every
    operation on its own, so that mask is theirs bit for bit, where two
    sets of statistics would flip an element within rounding of 0."""
    x, dy = case["x"].to(ct), case["dy"].to(ct)
    gamma, beta = case["gamma"].to(ct), case["beta"].to(ct)
    n = x.shape[0]
    mean = x.sum(0) / n
    m2 = ((x - mean) ** 2).sum(0)
    rstd = 1.0 / torch.sqrt(m2 / n + EPS)
    out = dict(mean=mean, rstd=rstd)
    out["running_mean"] = (1 - MOM) * case["rm"].to(ct) + MOM * mean
    out["running_var"] = (1 - MOM) * case["rv"].to(ct) + MOM * (m2 / (n - 1)) \
        if n > 1 else case["rv"].to(ct)
    y = ((x - mean) * rstd) * gamma + beta
    out["y"] = y.relu() if relu else y
    m32, r32 = stats if stats is not None else (mean.float(), rstd.float())
    xh = (x - m32.to(ct)) * r32.to(ct)
    g = dy
    if relu:
        pre32 = (case["x"].float() - m32) * r32 * case["gamma"] + case["beta"]
        g = torch.where(pre32 > 0, dy, torch.zeros_like(dy))
    out["dgamma"], out["dbeta"] = (g * xh).sum(0), g.sum(0)
    out["dx"] = (gamma * r32.to(ct)) * ((g - out["dbeta"] / n)
                                        - xh * (out["dgamma"] / n))
    return out


def _kernels(case, relu):
    _C = F._C
    assert F.has_ext(), "roc_amd._C must be built"
    x, dy = case["x"].to(DEV), case["dy"].to(DEV)
    gamma, beta = case["gamma"].to(DEV), case["beta"].to(DEV)
    rm, rv = case["rm"].to(DEV), case["rv"].to(DEV)
    n, D = x.shape
    mean, m2, rstd = (torch.empty(D, device=DEV) for _ in range(3))
    _C.batch_norm_stats(mean, m2, x)
    _C.batch_norm_finalize(rstd, mean, m2, rm, rv, n, MOM, EPS)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    _C.batch_norm_apply(y, x, mean, rstd, gamma, beta, relu)
    # poisoned: the fold overwrites, it does not accumulate
    dgamma = torch.full_like(gamma, float("nan"))
    dbeta = torch.full_like(beta, float("nan"))
    _C.batch_norm_bwd_reduce(dgamma, dbeta, dy, x, mean, rstd, gamma, beta,
                             relu)
    _C.batch_norm_bwd_dx(dx, dy, x, mean, rstd, gamma, beta, dbeta, dgamma,
                         n, relu)
    out = dict(mean=mean, m2=m2, rstd=rstd, running_mean=rm, running_var=rv,
               y=y, dx=dx, dgamma=dgamma, dbeta=dbeta)
    return {k: v.cpu() for k, v in out.items()}


def _check(got, want, figure, names, dtype):
    for k in names:
        g, w = got[k].double(), want[k]
        scale = w.abs().max().item()
        bound = 2 * figure[k] * scale + torch.zeros_like(w)
        if dtype == torch.bfloat16 and k in ("y", "dx"):
            assert got[k].dtype == dtype
            bound = bound + w.abs() * 2.0 ** -7
        err = (g - w).abs()
        print(f"{k}: err/scale {err.max().item() / max(scale, 1e-300):.3e} "
              f"(fp32 figure {figure[k]:.3e})")
        assert (err <= bound).all(), (k, err.max().item(), scale)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("N,D,dtype", CASES)
def test_kernels_against_fp64(N, D, dtype, relu):
    case = _case(N, D, dtype)
    got = _kernels(case, relu)
    want = _formulas(case, torch.float64, relu,
                     stats=(got["mean"], got["rstd"]))
    _check(got, want, FP32_FIGURE, list(FP32_FIGURE), dtype)


def test_shifted_sums_hold_a_large_offset():
    case = _case(40001, 64, torch.float32)
    gen = torch.Generator().manual_seed(5)
    case["x"] = 100.0 + 0.25 * torch.randn(40001, 64, generator=gen)
    got = _kernels(case, False)
    want = _formulas(case, torch.float64, False)
    _check(got, want, SHIFT_FIGURE, ["mean", "rstd"], torch.float32)


def test_constant_column_has_zero_m2():
    case = _case(3001, 16, torch.float32)
    case["x"][:, 2] = 3.25
    got = _kernels(case, False)
    assert got["m2"][2] == 0 and got["mean"][2] == 3.25
    assert got["rstd"][2] == 1.0 / torch.sqrt(torch.tensor(EPS))


@pytest.mark.parametrize("N,D,dtype", [(40001, 8, torch.float32),
                                       (3001, 520, torch.bfloat16)])
def test_two_runs_are_bit_identical(N, D, dtype):
    case = _case(N, D, dtype)
    a = _kernels(case, True)
    junk = torch.empty(12345, device=DEV)  # another allocation history
    b = _kernels(case, True)
    del junk
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_autograd_op_is_the_kernels():
    case = _case(1000, 40, torch.bfloat16)
    want = _kernels(case, True)
    leaves = [case[k].to(DEV).requires_grad_(True)
              for k in ("x", "gamma", "beta")]
    rm, rv = case["rm"].to(DEV), case["rv"].to(DEV)
    y = F.batch_norm(*leaves, rm, rv, training=True, momentum=MOM, eps=EPS,
                     activation="relu")
    y.backward(case["dy"].to(DEV))
    got = dict(y=y.detach(), dx=leaves[0].grad, dgamma=leaves[1].grad,
               dbeta=leaves[2].grad, running_mean=rm, running_var=rv)
    for k, v in got.items():
        assert torch.equal(v.cpu(), want[k]), k


# ---------------------------------------------------------------------------
# norm="sync_batch" through a GCN
# ---------------------------------------------------------------------------

def _trainer(device, dtype=torch.float32, capture=False):
    g, feats, labels, mask, c = synthetic_dataset("cora", scale=0.2, seed=7)
    feats = torch.nn.functional.pad(feats, (0, (-feats.shape[1]) % 8))
    model = build_model("gcn", [feats.shape[1], 64, 64, c], dropout=0.0,
                        seed=1, norm="sync_batch")
    opt = AdamOptimizer(model.parameters(), lr=0.01, weight_decay=1e-4,
                        no_decay=model.norm_parameters())
    tr = Trainer(model, build_shard(g, 0, 1), feats, labels, mask, opt,
                 device=device, compute_dtype=dtype, seed=11)
    if capture:
        tr.enable_graph_capture(warmup_epochs=2)
    return tr


def test_gcn_gpu_matches_cpu_path():
    tr_c, tr_g = _trainer("cpu"), _trainer(DEV)
    for _ in range(3):
        tr_c.train_epoch()
        tr_g.train_epoch()
    mc, mg = tr_c.evaluate(), tr_g.evaluate()
    assert mg["ce_loss"] == pytest.approx(mc["ce_loss"], rel=0.01)
    for i in range(2):
        for bc, bg in zip(running_stats(tr_c.model, i),
                          running_stats(tr_g.model, i)):
            assert torch.allclose(bc, bg.cpu(), rtol=1e-3, atol=1e-5)
    assert not torch.equal(tr_g.model.norm_running_var_0.cpu(),
                           torch.ones(64))


def test_capture_matches_eager(monkeypatch):
    """test_capture_matches_eager_with_layer_norm with norm="sync_batch": every
    replay advances the running buffers once, as every eager epoch does."""
    monkeypatch.setenv("ROC_DETERMINISTIC", "1")
    tr_e = _trainer(DEV, torch.bfloat16, capture=True)
    tr_e._graph_warmup = 10 ** 9  # device-schedule eager forever
    tr_g = _trainer(DEV, torch.bfloat16, capture=True)
    for _ in range(8):
        tr_e.train_epoch()
    for _ in range(8):
        tr_g.train_epoch()
    assert tr_e._graph is None and tr_g._graph is not None
    me, mg = tr_e.evaluate(), tr_g.evaluate()
    F.set_dropout_counter(None)
    pairs = [(tr_e.model.weights[0], tr_g.model.weights[0]),
             (tr_e.model.norm_gamma[0], tr_g.model.norm_gamma[0])]
    pairs += list(zip(running_stats(tr_e.model, 0),
                      running_stats(tr_g.model, 0)))
    for a, b in pairs:
        assert torch.allclose(a, b, atol=1e-5), (a - b).abs().max()
    assert mg["ce_loss"] == pytest.approx(me["ce_loss"], rel=0.01)
    assert tr_g.optimizer.t == tr_e.optimizer.t == 8


def test_errors_raise_before_any_launch():
    def t(n, d, dt=torch.float32):
        return torch.zeros(n, d, dtype=dt, device=DEV)

    def p(d):
        return torch.ones(d, device=DEV), torch.zeros(d, device=DEV)

    with pytest.raises(ValueError):
        F.batch_norm(t(4, 12, torch.bfloat16), *p(12))
    with pytest.raises(ValueError):
        F.batch_norm(t(4, 16, torch.float16), *p(16))
    with pytest.raises(ValueError):
        F.batch_norm(t(4, 16), torch.ones(15, device=DEV), p(16)[1])
    with pytest.raises(ValueError):
        F.batch_norm(t(4, 16), p(16)[0].bfloat16(), p(16)[1])
    with pytest.raises(ValueError):
        F.batch_norm(t(4, 16), *p(16), training=False)
    # the extension refuses the same on its own
    with pytest.raises(RuntimeError):
        F._C.batch_norm_stats(*p(12), t(4, 12, torch.bfloat16))
    with pytest.raises(RuntimeError):
        F._C.batch_norm_apply(t(4, 16), t(4, 16), *p(16), *p(15), False)
