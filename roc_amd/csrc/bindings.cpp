// Python bindings for the roc_amd CDNA4 kernel library (roc_amd._C).
#include <torch/extension.h>

void spmm(torch::Tensor out, torch::Tensor x, torch::Tensor rowptr,
          torch::Tensor colidx, c10::optional<torch::Tensor> deg_dst,
          c10::optional<torch::Tensor> deg_src,
          c10::optional<torch::Tensor> row_order, bool accumulate,
          int64_t col_base, int64_t ncols,
          c10::optional<torch::Tensor> heavy_rows, int64_t heavy_min,
          c10::optional<torch::Tensor> final_out);
void rowscale(torch::Tensor out, torch::Tensor x, torch::Tensor scale);
void cast_rowscale(torch::Tensor out, torch::Tensor x,
                   c10::optional<torch::Tensor> scale);
void relu_fwd(torch::Tensor out, torch::Tensor x);
void sigmoid_fwd(torch::Tensor out, torch::Tensor x);
void relu_bwd(torch::Tensor dx, torch::Tensor dy, torch::Tensor y);
void sigmoid_bwd(torch::Tensor dx, torch::Tensor dy, torch::Tensor y);
void ewise_add(torch::Tensor out, torch::Tensor a, torch::Tensor b);
void ewise_mul(torch::Tensor out, torch::Tensor a, torch::Tensor b);
void dropout_fwd(torch::Tensor out, torch::Tensor x, double p, int64_t seed,
                 int64_t offset, c10::optional<torch::Tensor> counter);
void softmax_ce(torch::Tensor dl, torch::Tensor metrics, torch::Tensor logits,
                torch::Tensor labels, torch::Tensor mask, double grad_scale,
                int64_t num_classes);
void adam_step(torch::Tensor w, torch::Tensor g, torch::Tensor m,
               torch::Tensor v, double alpha, double b1, double b2, double eps,
               double wd, c10::optional<torch::Tensor> step,
               double decay_rate, int64_t decay_steps);
void gemm_rr(torch::Tensor C, torch::Tensor A, torch::Tensor Bt, bool relu,
             c10::optional<torch::Tensor> row_scale);
void gemm_atb(torch::Tensor C, torch::Tensor A, torch::Tensor B);
void spmm_refresh_knobs();
void spmm_edge(torch::Tensor out, torch::Tensor x, torch::Tensor rowptr,
               torch::Tensor colidx, torch::Tensor edge_val,
               c10::optional<torch::Tensor> deg_dst,
               c10::optional<torch::Tensor> row_order, bool accumulate);
void edge_dot(torch::Tensor dw, torch::Tensor dy, torch::Tensor x,
              torch::Tensor rowptr, torch::Tensor colidx);
void seg_max_fwd(torch::Tensor out, c10::optional<torch::Tensor> arg,
                 torch::Tensor x, torch::Tensor rowptr, torch::Tensor colidx,
                 c10::optional<torch::Tensor> row_order, bool is_min);
void seg_max_bwd(torch::Tensor dx, torch::Tensor dy, torch::Tensor arg,
                 torch::Tensor t_rowptr, torch::Tensor t_colidx,
                 torch::Tensor t_eperm,
                 c10::optional<torch::Tensor> t_row_order);
void seg_stats_fwd(torch::Tensor out, c10::optional<torch::Tensor> stats,
                   c10::optional<torch::Tensor> arg, torch::Tensor x,
                   torch::Tensor rowptr, torch::Tensor colidx,
                   c10::optional<torch::Tensor> row_order, double eps,
                   int64_t depth);
void seg_stats_bwd(torch::Tensor dx, torch::Tensor dy, torch::Tensor x,
                   torch::Tensor stats, torch::Tensor arg,
                   torch::Tensor rowptr, torch::Tensor t_rowptr,
                   torch::Tensor t_colidx, torch::Tensor t_eperm,
                   c10::optional<torch::Tensor> t_row_order, int64_t depth);
void layer_norm_fwd(torch::Tensor y, c10::optional<torch::Tensor> mean,
                    c10::optional<torch::Tensor> rstd, torch::Tensor x,
                    torch::Tensor gamma, torch::Tensor beta, double eps,
                    bool relu);
void layer_norm_bwd(torch::Tensor dx, torch::Tensor dgamma,
                    torch::Tensor dbeta, torch::Tensor dy, torch::Tensor x,
                    torch::Tensor mean, torch::Tensor rstd,
                    torch::Tensor gamma, torch::Tensor beta, bool relu);
void graph_attn_fwd(torch::Tensor out, c10::optional<torch::Tensor> lse,
                    torch::Tensor q, torch::Tensor kv, torch::Tensor rowptr,
                    torch::Tensor colidx,
                    c10::optional<torch::Tensor> row_order, int64_t heads,
                    double scale);
void graph_attn_bwd_dst(torch::Tensor dq, torch::Tensor delta,
                        torch::Tensor dy, torch::Tensor out, torch::Tensor lse,
                        torch::Tensor q, torch::Tensor kv,
                        torch::Tensor rowptr, torch::Tensor colidx,
                        c10::optional<torch::Tensor> row_order, int64_t heads,
                        double scale);
void graph_attn_bwd_src(torch::Tensor dkv, torch::Tensor q, torch::Tensor dy,
                        torch::Tensor lse, torch::Tensor delta,
                        torch::Tensor kv, torch::Tensor t_rowptr,
                        torch::Tensor t_colidx,
                        c10::optional<torch::Tensor> t_row_order,
                        int64_t heads, double scale);
void edge_softmax_fwd(torch::Tensor alpha, torch::Tensor s,
                      torch::Tensor rowptr);
void edge_softmax_bwd(torch::Tensor ds, torch::Tensor dalpha,
                      torch::Tensor alpha, torch::Tensor rowptr);
void att_softmax_fwd(torch::Tensor alpha, torch::Tensor s_src,
                     torch::Tensor s_dst, torch::Tensor rowptr,
                     torch::Tensor colidx, double slope);
void att_softmax_bwd(torch::Tensor dsrc, torch::Tensor dsdst,
                     torch::Tensor dalpha, torch::Tensor alpha,
                     torch::Tensor s_src, torch::Tensor s_dst,
                     torch::Tensor rowptr, torch::Tensor colidx,
                     double slope);
void register_graph_cpu(pybind11::module_& m);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "roc_amd hand-written CDNA4 (gfx950) kernels";
  m.def("spmm", &spmm, "CSR SpMM neighbor aggregation (fused deg-norm)",
        pybind11::arg("out"), pybind11::arg("x"), pybind11::arg("rowptr"),
        pybind11::arg("colidx"), pybind11::arg("deg_dst") = pybind11::none(),
        pybind11::arg("deg_src") = pybind11::none(),
        pybind11::arg("row_order") = pybind11::none(),
        pybind11::arg("accumulate") = false,
        pybind11::arg("col_base") = 0, pybind11::arg("ncols") = 0,
        pybind11::arg("heavy_rows") = pybind11::none(),
        pybind11::arg("heavy_min") = 0,
        pybind11::arg("final_out") = pybind11::none());
  m.def("rowscale", &rowscale);
  m.def("cast_rowscale", &cast_rowscale,
        "fp32 -> bf16 cast with optional row scale (strip epilogue)",
        pybind11::arg("out"), pybind11::arg("x"),
        pybind11::arg("scale") = pybind11::none());
  m.def("relu_fwd", &relu_fwd);
  m.def("sigmoid_fwd", &sigmoid_fwd);
  m.def("relu_bwd", &relu_bwd);
  m.def("sigmoid_bwd", &sigmoid_bwd);
  m.def("ewise_add", &ewise_add);
  m.def("ewise_mul", &ewise_mul);
  m.def("dropout_fwd", &dropout_fwd, pybind11::arg("out"), pybind11::arg("x"),
        pybind11::arg("p"), pybind11::arg("seed"), pybind11::arg("offset"),
        pybind11::arg("counter") = pybind11::none());
  m.def("softmax_ce", &softmax_ce, pybind11::arg("dl"), pybind11::arg("metrics"),
        pybind11::arg("logits"), pybind11::arg("labels"), pybind11::arg("mask"),
        pybind11::arg("grad_scale"), pybind11::arg("num_classes") = -1);
  m.def("adam_step", &adam_step, pybind11::arg("w"), pybind11::arg("g"),
        pybind11::arg("m"), pybind11::arg("v"), pybind11::arg("alpha"),
        pybind11::arg("b1"), pybind11::arg("b2"), pybind11::arg("eps"),
        pybind11::arg("wd"), pybind11::arg("step") = pybind11::none(),
        pybind11::arg("decay_rate") = 1.0,
        pybind11::arg("decay_steps") = 100);
  m.def("gemm_rr", &gemm_rr, "C = A @ Bt^T (bf16 MFMA, fused relu/rowscale)",
        pybind11::arg("C"), pybind11::arg("A"), pybind11::arg("Bt"),
        pybind11::arg("relu"), pybind11::arg("row_scale") = pybind11::none());
  m.def("gemm_atb", &gemm_atb, "C += A^T @ B (fp32 split-K accumulate)");
  m.def("spmm_refresh_knobs", &spmm_refresh_knobs,
        "re-read ROC_SPMM_* env knobs (A/B harness only)");
  m.def("spmm_edge", &spmm_edge,
        "per-edge-weighted CSR SpMM (edge-tensor consumer)",
        pybind11::arg("out"), pybind11::arg("x"), pybind11::arg("rowptr"),
        pybind11::arg("colidx"), pybind11::arg("edge_val"),
        pybind11::arg("deg_dst") = pybind11::none(),
        pybind11::arg("row_order") = pybind11::none(),
        pybind11::arg("accumulate") = false);
  m.def("edge_dot", &edge_dot,
        "dw[e] = <dy[row_e], x[col_e]> (edge-value gradient)");
  m.def("seg_max_fwd", &seg_max_fwd,
        "CSR segment max/min aggregation; arg = winning forward edge index",
        pybind11::arg("out"), pybind11::arg("arg"), pybind11::arg("x"),
        pybind11::arg("rowptr"), pybind11::arg("colidx"),
        pybind11::arg("row_order") = pybind11::none(),
        pybind11::arg("is_min") = false);
  m.def("seg_max_bwd", &seg_max_bwd,
        "segment max/min gradient: gather of dy over the transpose CSR",
        pybind11::arg("dx"), pybind11::arg("dy"), pybind11::arg("arg"),
        pybind11::arg("t_rowptr"), pybind11::arg("t_colidx"),
        pybind11::arg("t_eperm"),
        pybind11::arg("t_row_order") = pybind11::none());
  m.def("seg_stats_fwd", &seg_stats_fwd,
        "CSR segment mean/std/max/min in one gather: out = [mean|std|max|min],"
        " stats = fp32 [mean|1/std], arg = [argmax|argmin] forward edges; "
        "stats = arg = None skips their stores",
        pybind11::arg("out"), pybind11::arg("stats"), pybind11::arg("arg"),
        pybind11::arg("x"), pybind11::arg("rowptr"), pybind11::arg("colidx"),
        pybind11::arg("row_order") = pybind11::none(),
        pybind11::arg("eps") = 1e-5, pybind11::arg("depth") = 0);
  m.def("seg_stats_bwd", &seg_stats_bwd,
        "seg_stats gradient: one gather of stats, dy and arg over the "
        "transpose CSR",
        pybind11::arg("dx"), pybind11::arg("dy"), pybind11::arg("x"),
        pybind11::arg("stats"), pybind11::arg("arg"),
        pybind11::arg("rowptr"), pybind11::arg("t_rowptr"),
        pybind11::arg("t_colidx"),
        pybind11::arg("t_eperm"),
        pybind11::arg("t_row_order") = pybind11::none(),
        pybind11::arg("depth") = 0);
  m.def("layer_norm_fwd", &layer_norm_fwd,
        "per-row LayerNorm (+ReLU); mean = rstd = None skips the stats stores",
        pybind11::arg("y"), pybind11::arg("mean"), pybind11::arg("rstd"),
        pybind11::arg("x"), pybind11::arg("gamma"), pybind11::arg("beta"),
        pybind11::arg("eps"), pybind11::arg("relu") = false);
  m.def("layer_norm_bwd", &layer_norm_bwd,
        "LayerNorm gradient: dx, and dgamma / dbeta by an order-fixed slab fold",
        pybind11::arg("dx"), pybind11::arg("dgamma"), pybind11::arg("dbeta"),
        pybind11::arg("dy"), pybind11::arg("x"), pybind11::arg("mean"),
        pybind11::arg("rstd"), pybind11::arg("gamma"), pybind11::arg("beta"),
        pybind11::arg("relu") = false);
  m.def("graph_attn_fwd", &graph_attn_fwd,
        "dot-product attention over in-neighbours (online softmax); "
        "lse = None skips the log-sum-exp store",
        pybind11::arg("out"), pybind11::arg("lse"), pybind11::arg("q"),
        pybind11::arg("kv"), pybind11::arg("rowptr"), pybind11::arg("colidx"),
        pybind11::arg("row_order"), pybind11::arg("heads"),
        pybind11::arg("scale"));
  m.def("graph_attn_bwd_dst", &graph_attn_bwd_dst,
        "attention gradient, destination-major pass: delta and dq",
        pybind11::arg("dq"), pybind11::arg("delta"), pybind11::arg("dy"),
        pybind11::arg("out"), pybind11::arg("lse"), pybind11::arg("q"),
        pybind11::arg("kv"), pybind11::arg("rowptr"), pybind11::arg("colidx"),
        pybind11::arg("row_order"), pybind11::arg("heads"),
        pybind11::arg("scale"));
  m.def("graph_attn_bwd_src", &graph_attn_bwd_src,
        "attention gradient, source-major pass over the transpose CSR: dkv",
        pybind11::arg("dkv"), pybind11::arg("q"), pybind11::arg("dy"),
        pybind11::arg("lse"), pybind11::arg("delta"), pybind11::arg("kv"),
        pybind11::arg("t_rowptr"), pybind11::arg("t_colidx"),
        pybind11::arg("t_row_order"), pybind11::arg("heads"),
        pybind11::arg("scale"));
  m.def("edge_softmax_fwd", &edge_softmax_fwd,
        "per-row segment softmax over edge scores (GAT attention)");
  m.def("edge_softmax_bwd", &edge_softmax_bwd);
  m.def("att_softmax_fwd", &att_softmax_fwd,
        "fused GAT attention: lrelu(s_src[col]+s_dst[row]) -> softmax");
  m.def("att_softmax_bwd", &att_softmax_bwd);
  register_graph_cpu(m);
}
