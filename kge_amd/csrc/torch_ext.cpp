// torch_ext.cpp -- the PyTorch-ROCm C++ extension over the C ABI (include/kge_amd.h): `kge_amd._C`.
//
// north_star asks for the engine "exposed through a PyTorch-ROCm C++/HIP extension that keeps the RelationalScorer /
// KgeModel plugin API".  The kernels and the drop-in boundary stay in libkge_amd.so (plain C, no torch types); this
// file is the thin torch side of it: tensors in, tensors out, outputs from torch's caching allocator, launches on
// torch's CURRENT HIP stream, C status codes turned into TORCH_CHECK failures (RuntimeError in Python).  An allocation
// failure of an output is re-raised as RuntimeError("CUDA out of memory ...") -- on ROCm torch's own text is "HIP out
// of memory", and the reference's sub-batch auto-tuner string-matches the CUDA spelling (kge/job/train.py:384-391):
// `empty_f32` below; tests/test_gpu_queries.py::test_out_of_memory_keeps_the_text_the_reference_greps_for.
// One C++ call per scoring call instead of a ctypes call with a dozen boxed arguments: ~2 us of host time instead of ~9
// (tools/host_overhead.py).
//
// Mirrors (paths in the reference tree):
//   score_spo / score_sp / score_po / score_sp_po   KgeModel.score_*      kge/model/kge_model.py:663-789
//   build_queries_group / score_queries_group       the same scores for a GROUP of batches in one persistent launch
//   topk                                            score_sp / score_po + the masking of _filter_and_rank
//                                                   (kge/job/eval_entity_ranking.py:233-313) + torch.topk
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include <vector>

#include "../../include/kge_amd.h"

namespace {

void check(int rc, const char* what) {
  TORCH_CHECK(rc == KGE_OK, "kge_amd: ", what, " failed: ", kge_status_string(rc), " (kge_status ", rc, ")");
}

// Output allocation through torch's caching allocator with the reference's OOM text (SURVEY.md 8b "Error conventions").
at::Tensor empty_f32(at::IntArrayRef shape, const at::Tensor& like) {
  try {
    return at::empty(shape, like.options().dtype(at::kFloat));
  } catch (const c10::OutOfMemoryError& e) {
    TORCH_CHECK(false, "CUDA out of memory (kge_amd, ROCm: ", e.what_without_backtrace(), ")");
  }
  return at::Tensor();  // not reached
}

void* stream_of(const at::Tensor& t) { return (void*)c10::hip::getCurrentHIPStream(t.get_device()).stream(); }

kge_tables tables_of(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm, int64_t flags) {
  TORCH_CHECK(ent.is_cuda() && rel.is_cuda() && ent.get_device() == rel.get_device(),
              "kge_amd: embedding tables must live on one GPU (no CPU path)");
  TORCH_CHECK(ent.dim() == 2 && rel.dim() == 2 && ent.stride(1) == 1 && rel.stride(1) == 1, "kge_amd: tables are [rows, dim]");
  TORCH_CHECK(ent.scalar_type() == rel.scalar_type() &&
                  (ent.scalar_type() == at::kFloat || ent.scalar_type() == at::kBFloat16),
              "kge_amd: tables must be float32 or bfloat16");
  kge_tables t{};
  t.ent = ent.data_ptr();
  t.rel = rel.data_ptr();
  t.dtype = ent.scalar_type() == at::kBFloat16 ? KGE_BF16 : KGE_F32;
  t.scorer = (int32_t)scorer;
  t.num_ent = ent.size(0);
  t.num_rel = rel.size(0);
  t.dim = ent.size(1);
  t.rel_dim = rel.size(1);
  t.ent_ld = ent.stride(0);
  t.rel_ld = rel.stride(0);
  t.l_norm = (float)l_norm;
  t.flags = (int32_t)flags;
  return t;
}

// 1-D int32 / int64 index tensor of any stride (the trainers pass triples[:, k]); anything else is converted (kept alive)
kge_index index_of(const c10::optional<at::Tensor>& ix, const at::Tensor& like, std::vector<at::Tensor>& keep, int64_t* n) {
  kge_index k{nullptr, KGE_I64, 0, 1};
  if (!ix.has_value() || !ix->defined()) return k;
  at::Tensor t = *ix;
  TORCH_CHECK(t.is_cuda() && t.get_device() == like.get_device(), "kge_amd: index tensor on ", t.device(), ", tables on ",
              like.device());
  if (t.dim() != 1) t = t.reshape({-1});
  if (t.scalar_type() != at::kInt && t.scalar_type() != at::kLong) t = t.to(at::kLong);
  int64_t stride = t.numel() > 1 ? t.stride(0) : 1;
  if (stride < 1) {
    t = t.contiguous();
    stride = 1;
  }
  keep.push_back(t);
  k.ptr = t.data_ptr();
  k.itype = t.scalar_type() == at::kInt ? KGE_I32 : KGE_I64;
  k.stride = stride;
  if (n != nullptr) {
    TORCH_CHECK_VALUE(*n < 0 || *n == t.numel(), "kge_amd: index vectors of different lengths (", *n, " and ", t.numel(), ")");
    *n = t.numel();
  }
  return k;
}

at::Tensor score_spo(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm, int64_t flags,
                     const at::Tensor& s, const at::Tensor& p, const at::Tensor& o) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, flags);
  std::vector<at::Tensor> keep;
  int64_t n = -1;
  const kge_index si = index_of(s, ent, keep, &n), pi = index_of(p, ent, keep, &n), oi = index_of(o, ent, keep, &n);
  at::Tensor out = empty_f32({n}, ent);
  check(kge_score_spo(&t, si, pi, oi, n, out.data_ptr<float>(), stream_of(ent)), "kge_score_spo");
  return out;
}

// KgeModel.score_so (kge_model.py:727-747): [n, m] scores of (s[i], rels[j], o[i]); rels absent = all relations
at::Tensor score_so(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm, int64_t flags,
                    const at::Tensor& s, const at::Tensor& o, const c10::optional<at::Tensor>& rels) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, flags);
  std::vector<at::Tensor> keep;
  int64_t n = -1, m = -1;
  const kge_index si = index_of(s, ent, keep, &n), oi = index_of(o, ent, keep, &n);
  const kge_index ri = index_of(rels, ent, keep, &m);
  if (m < 0) m = t.num_rel;
  at::Tensor out = empty_f32({n, m}, ent);
  check(kge_score_so(&t, si, oi, n, ri, m, out.data_ptr<float>(), m > 0 ? m : 1, nullptr, 0, stream_of(ent)),
        "kge_score_so");
  return out;
}

// its backward, accumulated into the dense float32 table gradients; false where the kernel declines the tables
bool score_so_bwd_accum(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm, const at::Tensor& s,
                        const at::Tensor& o, const c10::optional<at::Tensor>& rels, const at::Tensor& gout,
                        const c10::optional<at::Tensor>& scores, at::Tensor grad_ent, at::Tensor grad_rel) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, 0);
  std::vector<at::Tensor> keep;
  int64_t n = -1, m = -1;
  const kge_index si = index_of(s, ent, keep, &n), oi = index_of(o, ent, keep, &n);
  const kge_index ri = index_of(rels, ent, keep, &m);
  if (m < 0) m = t.num_rel;
  const bool has_sc = scores.has_value() && scores->defined();
  TORCH_CHECK(gout.is_cuda() && gout.scalar_type() == at::kFloat && gout.dim() == 2 && gout.size(0) == n &&
                  gout.size(1) == m && (m <= 1 || gout.stride(1) == 1),
              "kge_amd: score_so_bwd_accum: gout is an [n, m] float32 GPU tensor with unit inner stride");
  TORCH_CHECK(!has_sc || (scores->is_cuda() && scores->scalar_type() == at::kFloat && scores->dim() == 2 &&
                          scores->size(0) == n && scores->size(1) == m && (m <= 1 || scores->stride(1) == 1)),
              "kge_amd: score_so_bwd_accum: scores is an [n, m] float32 GPU tensor with unit inner stride");
  for (const at::Tensor* g : {&grad_ent, &grad_rel})
    TORCH_CHECK(g->is_cuda() && g->scalar_type() == at::kFloat && g->dim() == 2 && g->stride(1) == 1,
                "kge_amd: score_so_bwd_accum: the table gradients are float32 GPU matrices");
  TORCH_CHECK(grad_ent.size(0) == ent.size(0) && grad_ent.size(1) == ent.size(1) && grad_rel.size(0) == rel.size(0) &&
                  grad_rel.size(1) == rel.size(1),
              "kge_amd: score_so_bwd_accum: the table gradients have the tables' shapes");
  const int64_t one = m > 0 ? m : 1;
  const int rc = kge_score_so_bwd_accum(&t, si, oi, n, ri, m, gout.data_ptr<float>(), n > 1 ? gout.stride(0) : one,
                                        has_sc ? scores->data_ptr<float>() : nullptr,
                                        has_sc ? (n > 1 ? scores->stride(0) : one) : 0, grad_ent.data_ptr<float>(),
                                        grad_ent.stride(0), grad_rel.data_ptr<float>(), grad_rel.stride(0), nullptr, 0,
                                        stream_of(ent));
  if (rc == KGE_ERR_UNSUPPORTED) return false;
  check(rc, "kge_score_so_bwd_accum");
  return true;
}

// combine: 1 = sp_ (a = s), 2 = _po (a = o), 3 = both blocks [n, 2 m] (a = s, b = o)
at::Tensor score_pairs(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm, int64_t flags,
                       int64_t combine, const at::Tensor& a, const at::Tensor& p, const c10::optional<at::Tensor>& b,
                       const c10::optional<at::Tensor>& targets, const c10::optional<at::Tensor>& workspace) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, flags);
  std::vector<at::Tensor> keep;
  int64_t n = -1, m = -1;
  const kge_index ai = index_of(a, ent, keep, &n), pi = index_of(p, ent, keep, &n);
  const kge_index bi = combine == KGE_SP_PO ? index_of(b, ent, keep, &n) : kge_index{nullptr, KGE_I64, 0, 1};
  const kge_index ti = index_of(targets, ent, keep, &m);
  if (m < 0) m = t.num_ent;
  void* ws = nullptr;
  int64_t wsb = 0;
  if (workspace.has_value() && workspace->defined()) {
    TORCH_CHECK(workspace->is_cuda() && workspace->is_contiguous(), "kge_amd: workspace must be a contiguous GPU tensor");
    ws = workspace->data_ptr();
    wsb = workspace->numel() * workspace->element_size();
  }
  const int64_t width = combine == KGE_SP_PO ? 2 * m : m;
  at::Tensor out = empty_f32({n, width}, ent);
  const int64_t ldo = width > 0 ? width : 1;
  void* st = stream_of(ent);
  if (combine == KGE_SP_)
    check(kge_score_sp(&t, ai, pi, n, ti, m, out.data_ptr<float>(), ldo, ws, wsb, st), "kge_score_sp");
  else if (combine == KGE_PO_)
    check(kge_score_po(&t, pi, ai, n, ti, m, out.data_ptr<float>(), ldo, ws, wsb, st), "kge_score_po");
  else if (combine == KGE_SP_PO)
    check(kge_score_sp_po(&t, ai, pi, bi, n, ti, m, out.data_ptr<float>(), ldo, ws, wsb, st), "kge_score_sp_po");
  else
    TORCH_CHECK(false, "kge_amd: combine must be 1 (sp_), 2 (_po) or 3 (sp_po)");
  return out;
}

int64_t queries_bytes(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, int64_t flags, int64_t combine, int64_t n) {
  const kge_tables t = tables_of(ent, rel, scorer, 1.0, flags);
  return kge_queries_bytes(&t, (int)combine, n);
}

void build_queries_group(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, int64_t flags, int64_t combine,
                         const c10::optional<at::Tensor>& s, const at::Tensor& p, const c10::optional<at::Tensor>& o,
                         int64_t n, int64_t num_batches, const at::Tensor& queries, int64_t stride) {
  const kge_tables t = tables_of(ent, rel, scorer, 1.0, flags);
  std::vector<at::Tensor> keep;
  int64_t len = -1;
  const kge_index si = index_of(s, ent, keep, &len), pi = index_of(p, ent, keep, &len), oi = index_of(o, ent, keep, &len);
  TORCH_CHECK_VALUE(len == n * num_batches, "kge_amd: a group of ", num_batches, " batches of ", n, " rows needs ", n * num_batches,
              " index entries, got ", len);
  TORCH_CHECK(queries.is_cuda() && queries.is_contiguous() && queries.scalar_type() == at::kByte, "kge_amd: queries buffer");
  check(kge_build_queries_multi(&t, (int)combine, si, pi, oi, n, num_batches, queries.data_ptr(), stride, queries.numel(),
                                stream_of(ent)),
        "kge_build_queries_multi");
}

// out: [L, n, m] / [L, n, 2 m] (any row pitch, unit inner stride) or [L, n, 2, m]
// next_*: the NEXT group's index vectors (num_batches * next_n entries each) and fragment buffer -- built by the same
// launch behind its last unit (kge_next_queries); next_queries undefined: none
void score_queries_group(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, int64_t flags, int64_t combine,
                         const at::Tensor& queries, int64_t stride, int64_t n, int64_t num_batches, at::Tensor out,
                         const c10::optional<at::Tensor>& next_s, const c10::optional<at::Tensor>& next_p,
                         const c10::optional<at::Tensor>& next_o, int64_t next_n,
                         const c10::optional<at::Tensor>& next_queries, int64_t next_stride) {
  const kge_tables t = tables_of(ent, rel, scorer, 1.0, flags);
  const int64_t m = t.num_ent;
  TORCH_CHECK_VALUE(out.is_cuda() && out.get_device() == ent.get_device() && out.scalar_type() == at::kFloat,
                    "kge_amd: `out` must be a float32 tensor on the tables' GPU");
  TORCH_CHECK_VALUE(out.dim() >= 3 && out.size(0) == num_batches && out.size(1) == n, "kge_amd: `out` is [L, n, ...]");
  int64_t ldo = out.stride(1), b2 = 0;
  const int64_t width = combine == KGE_SP_PO ? 2 * m : m;
  if (out.dim() == 4) {
    TORCH_CHECK_VALUE(combine == KGE_SP_PO && out.size(2) == 2 && out.size(3) == m && (m <= 1 || out.stride(3) == 1) &&
                    out.stride(2) >= m,
                "kge_amd: a 4-D `out` is [L, n, 2, m] with unit inner stride");
    b2 = out.stride(2);
  } else {
    TORCH_CHECK_VALUE(out.dim() == 3 && out.size(2) == width && (width <= 1 || out.stride(2) == 1),
                "kge_amd: `out` must be [L, n, ", width, "] with unit inner stride");
  }
  const int64_t need = b2 > 0 ? b2 + m : width;
  if (n == 1 && ldo < need) ldo = need;
  TORCH_CHECK_VALUE(ldo >= need, "kge_amd: the rows of `out` overlap");
  kge_index all{nullptr, KGE_I64, 0, 1};
  kge_next_queries nx{};
  const kge_next_queries* nxp = nullptr;
  std::vector<at::Tensor> keep;
  if (next_queries.has_value() && next_queries->defined() && next_n > 0) {
    const at::Tensor& nq = *next_queries;
    TORCH_CHECK_VALUE(nq.is_cuda() && nq.is_contiguous() && nq.scalar_type() == at::kByte, "kge_amd: next_queries buffer");
    int64_t len = -1;
    nx.s = index_of(next_s, ent, keep, &len);
    nx.p = index_of(next_p, ent, keep, &len);
    nx.o = index_of(next_o, ent, keep, &len);
    TORCH_CHECK_VALUE(len == next_n * num_batches, "kge_amd: the next group needs ", next_n * num_batches, " index entries, got ",
                      len);
    nx.n = next_n;
    nx.queries = nq.data_ptr();
    nx.queries_bytes = nq.numel();
    nxp = &nx;
  }
  check(kge_score_queries_multi(&t, (int)combine, queries.data_ptr(), stride, n, num_batches, all, m, out.data_ptr<float>(),
                                num_batches > 1 ? out.stride(0) : 0, ldo, b2, nxp, nxp ? next_stride : 0, stream_of(ent)),
        "kge_score_queries_multi");
}

// ---- fused 1vsAll loss of TransE / RotatE on float32 tables (kge_ce_dist_*; direction: 1 = sp_, 2 = _po).  The
// workspace is the caller's (engine.py caches one per device and stream); its first `workspace_bytes` bytes are used.
int64_t ce_dist_workspace_bytes(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm, int64_t n,
                                int64_t chunk_cols) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, 0);
  return kge_ce_dist_workspace_bytes(&t, n, chunk_cols);
}

void* ce_dist_ws(const at::Tensor& workspace, int64_t workspace_bytes) {
  TORCH_CHECK(workspace.is_cuda() && workspace.is_contiguous() &&
                  workspace.numel() * workspace.element_size() >= workspace_bytes,
              "kge_amd: workspace must be a contiguous GPU tensor of at least workspace_bytes bytes");
  return workspace.data_ptr();
}

std::vector<at::Tensor> ce_dist_fwd(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm,
                                    int64_t direction, const at::Tensor& a, const at::Tensor& p, const at::Tensor& label,
                                    const at::Tensor& workspace, int64_t workspace_bytes) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, 0);
  std::vector<at::Tensor> keep;
  int64_t n = -1;
  const kge_index ai = index_of(a, ent, keep, &n), pi = index_of(p, ent, keep, &n), li = index_of(label, ent, keep, &n);
  at::Tensor loss_rows = empty_f32({n}, ent), lse = empty_f32({n}, ent);
  check(kge_ce_dist_fwd(&t, (int)direction, ai, pi, li, n, loss_rows.data_ptr<float>(), lse.data_ptr<float>(),
                        ce_dist_ws(workspace, workspace_bytes), workspace_bytes, stream_of(ent)),
        "kge_ce_dist_fwd");
  return {loss_rows, lse};
}

std::vector<at::Tensor> ce_dist_bwd(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm,
                                    int64_t direction, const at::Tensor& a, const at::Tensor& p, const at::Tensor& label,
                                    const at::Tensor& lse, const c10::optional<at::Tensor>& g_rows, double g_scalar,
                                    const at::Tensor& workspace, int64_t workspace_bytes) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, 0);
  std::vector<at::Tensor> keep;
  int64_t n = -1;
  const kge_index ai = index_of(a, ent, keep, &n), pi = index_of(p, ent, keep, &n), li = index_of(label, ent, keep, &n);
  const at::Tensor lse_c = lse.to(at::kFloat).contiguous();
  TORCH_CHECK_VALUE(lse_c.numel() == n, "kge_amd: lse must have one entry per row");
  at::Tensor gr;
  if (g_rows.has_value() && g_rows->defined()) {
    gr = g_rows->to(at::kFloat).contiguous();
    TORCH_CHECK_VALUE(gr.numel() == n, "kge_amd: g_rows must have one entry per row");
  }
  at::Tensor g_a = empty_f32({n, t.dim}, ent), g_p = empty_f32({n, t.rel_dim}, ent), g_t = empty_f32({t.num_ent, t.dim}, ent);
  check(kge_ce_dist_bwd(&t, (int)direction, ai, pi, li, n, lse_c.data_ptr<float>(),
                        gr.defined() ? gr.data_ptr<float>() : nullptr, (float)g_scalar, g_a.data_ptr<float>(),
                        g_p.data_ptr<float>(), g_t.data_ptr<float>(), ce_dist_ws(workspace, workspace_bytes),
                        workspace_bytes, stream_of(ent)),
        "kge_ce_dist_bwd");
  return {g_a, g_p, g_t};
}

// ---- fused 1vsAll loss of ComplEx / DistMult on FLOAT32 tables (kge_ce_f32_*): the same signatures; l_norm is not read
int64_t ce_f32_workspace_bytes(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm, int64_t n,
                                int64_t chunk_cols) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, 0);
  return kge_ce_f32_workspace_bytes(&t, n, chunk_cols);
}

std::vector<at::Tensor> ce_f32_fwd(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm,
                                    int64_t direction, const at::Tensor& a, const at::Tensor& p, const at::Tensor& label,
                                    const at::Tensor& workspace, int64_t workspace_bytes) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, 0);
  std::vector<at::Tensor> keep;
  int64_t n = -1;
  const kge_index ai = index_of(a, ent, keep, &n), pi = index_of(p, ent, keep, &n), li = index_of(label, ent, keep, &n);
  at::Tensor loss_rows = empty_f32({n}, ent), lse = empty_f32({n}, ent);
  check(kge_ce_f32_fwd(&t, (int)direction, ai, pi, li, n, loss_rows.data_ptr<float>(), lse.data_ptr<float>(),
                        ce_dist_ws(workspace, workspace_bytes), workspace_bytes, stream_of(ent)),
        "kge_ce_f32_fwd");
  return {loss_rows, lse};
}

std::vector<at::Tensor> ce_f32_bwd(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm,
                                    int64_t direction, const at::Tensor& a, const at::Tensor& p, const at::Tensor& label,
                                    const at::Tensor& lse, const c10::optional<at::Tensor>& g_rows, double g_scalar,
                                    const at::Tensor& workspace, int64_t workspace_bytes) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, 0);
  std::vector<at::Tensor> keep;
  int64_t n = -1;
  const kge_index ai = index_of(a, ent, keep, &n), pi = index_of(p, ent, keep, &n), li = index_of(label, ent, keep, &n);
  const at::Tensor lse_c = lse.to(at::kFloat).contiguous();
  TORCH_CHECK_VALUE(lse_c.numel() == n, "kge_amd: lse must have one entry per row");
  at::Tensor gr;
  if (g_rows.has_value() && g_rows->defined()) {
    gr = g_rows->to(at::kFloat).contiguous();
    TORCH_CHECK_VALUE(gr.numel() == n, "kge_amd: g_rows must have one entry per row");
  }
  at::Tensor g_a = empty_f32({n, t.dim}, ent), g_p = empty_f32({n, t.rel_dim}, ent), g_t = empty_f32({t.num_ent, t.dim}, ent);
  check(kge_ce_f32_bwd(&t, (int)direction, ai, pi, li, n, lse_c.data_ptr<float>(),
                        gr.defined() ? gr.data_ptr<float>() : nullptr, (float)g_scalar, g_a.data_ptr<float>(),
                        g_p.data_ptr<float>(), g_t.data_ptr<float>(), ce_dist_ws(workspace, workspace_bytes),
                        workspace_bytes, stream_of(ent)),
        "kge_ce_f32_bwd");
  return {g_a, g_p, g_t};
}

// ---- the KvsAll losses of TransE / RotatE on float32 tables (kge_kl_dist_* / kge_bce_dist_*): labels as an int64 CSR
// (rowptr [n + 1], col [nnz]) on the tables' device; workspace as above (kge_multilabel_dist_workspace_bytes).
int64_t multilabel_dist_workspace_bytes(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm,
                                        int64_t n, int64_t chunk_cols) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, 0);
  return kge_multilabel_dist_workspace_bytes(&t, n, chunk_cols);
}

struct DistLabels {
  at::Tensor rowptr, col, weight, g_rows;
  const float* w = nullptr;
  const float* g = nullptr;
};

DistLabels dist_labels(const at::Tensor& ent, int64_t n, const at::Tensor& rowptr, const at::Tensor& col,
                       const c10::optional<at::Tensor>& weight, const c10::optional<at::Tensor>& g_rows) {
  DistLabels l;
  TORCH_CHECK(rowptr.is_cuda() && col.is_cuda() && rowptr.get_device() == ent.get_device() &&
                  col.get_device() == ent.get_device(), "kge_amd: the label CSR must live on the tables' device");
  l.rowptr = rowptr.to(at::kLong).contiguous();
  l.col = col.to(at::kLong).contiguous();
  if (l.col.numel() == 0) l.col = at::zeros({1}, l.col.options());
  TORCH_CHECK_VALUE(l.rowptr.numel() == n + 1, "kge_amd: label rowptr has ", l.rowptr.numel(), " entries for ", n, " rows");
  if (weight.has_value() && weight->defined()) {
    l.weight = weight->to(at::kFloat).contiguous();
    TORCH_CHECK_VALUE(l.weight.numel() == n, "kge_amd: label_weight must have one entry per row");
    l.w = l.weight.data_ptr<float>();
  }
  if (g_rows.has_value() && g_rows->defined()) {
    l.g_rows = g_rows->to(at::kFloat).contiguous();
    TORCH_CHECK_VALUE(l.g_rows.numel() == n, "kge_amd: g_rows must have one entry per row");
    l.g = l.g_rows.data_ptr<float>();
  }
  return l;
}

std::vector<at::Tensor> kl_dist_fwd(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm,
                                    int64_t direction, const at::Tensor& a, const at::Tensor& p, const at::Tensor& rowptr,
                                    const at::Tensor& col, const c10::optional<at::Tensor>& label_weight,
                                    const at::Tensor& workspace, int64_t workspace_bytes) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, 0);
  std::vector<at::Tensor> keep;
  int64_t n = -1;
  const kge_index ai = index_of(a, ent, keep, &n), pi = index_of(p, ent, keep, &n);
  const DistLabels l = dist_labels(ent, n, rowptr, col, label_weight, c10::nullopt);
  at::Tensor loss_rows = empty_f32({n}, ent), lse = empty_f32({n}, ent);
  check(kge_kl_dist_fwd(&t, (int)direction, ai, pi, n, l.rowptr.data_ptr<int64_t>(), l.col.data_ptr<int64_t>(), l.w,
                        loss_rows.data_ptr<float>(), lse.data_ptr<float>(), ce_dist_ws(workspace, workspace_bytes),
                        workspace_bytes, stream_of(ent)),
        "kge_kl_dist_fwd");
  return {loss_rows, lse};
}

std::vector<at::Tensor> kl_dist_bwd(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm,
                                    int64_t direction, const at::Tensor& a, const at::Tensor& p, const at::Tensor& rowptr,
                                    const at::Tensor& col, const c10::optional<at::Tensor>& label_weight,
                                    const at::Tensor& lse, const c10::optional<at::Tensor>& g_rows, double g_scalar,
                                    const at::Tensor& workspace, int64_t workspace_bytes) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, 0);
  std::vector<at::Tensor> keep;
  int64_t n = -1;
  const kge_index ai = index_of(a, ent, keep, &n), pi = index_of(p, ent, keep, &n);
  const DistLabels l = dist_labels(ent, n, rowptr, col, label_weight, g_rows);
  const at::Tensor lse_c = lse.to(at::kFloat).contiguous();
  TORCH_CHECK_VALUE(lse_c.numel() == n, "kge_amd: lse must have one entry per row");
  at::Tensor g_a = empty_f32({n, t.dim}, ent), g_p = empty_f32({n, t.rel_dim}, ent), g_t = empty_f32({t.num_ent, t.dim}, ent);
  check(kge_kl_dist_bwd(&t, (int)direction, ai, pi, n, l.rowptr.data_ptr<int64_t>(), l.col.data_ptr<int64_t>(), l.w,
                        lse_c.data_ptr<float>(), l.g, (float)g_scalar, g_a.data_ptr<float>(), g_p.data_ptr<float>(),
                        g_t.data_ptr<float>(), ce_dist_ws(workspace, workspace_bytes), workspace_bytes, stream_of(ent)),
        "kge_kl_dist_bwd");
  return {g_a, g_p, g_t};
}

at::Tensor bce_dist_fwd(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm, int64_t direction,
                        const at::Tensor& a, const at::Tensor& p, const at::Tensor& rowptr, const at::Tensor& col,
                        double offset, const at::Tensor& workspace, int64_t workspace_bytes) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, 0);
  std::vector<at::Tensor> keep;
  int64_t n = -1;
  const kge_index ai = index_of(a, ent, keep, &n), pi = index_of(p, ent, keep, &n);
  const DistLabels l = dist_labels(ent, n, rowptr, col, c10::nullopt, c10::nullopt);
  at::Tensor loss_rows = empty_f32({n}, ent);
  check(kge_bce_dist_fwd(&t, (int)direction, ai, pi, n, l.rowptr.data_ptr<int64_t>(), l.col.data_ptr<int64_t>(),
                         (float)offset, loss_rows.data_ptr<float>(), ce_dist_ws(workspace, workspace_bytes),
                         workspace_bytes, stream_of(ent)),
        "kge_bce_dist_fwd");
  return loss_rows;
}

std::vector<at::Tensor> bce_dist_bwd(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm,
                                     int64_t direction, const at::Tensor& a, const at::Tensor& p, const at::Tensor& rowptr,
                                     const at::Tensor& col, double offset, const c10::optional<at::Tensor>& g_rows,
                                     double g_scalar, const at::Tensor& workspace, int64_t workspace_bytes) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, 0);
  std::vector<at::Tensor> keep;
  int64_t n = -1;
  const kge_index ai = index_of(a, ent, keep, &n), pi = index_of(p, ent, keep, &n);
  const DistLabels l = dist_labels(ent, n, rowptr, col, c10::nullopt, g_rows);
  at::Tensor g_a = empty_f32({n, t.dim}, ent), g_p = empty_f32({n, t.rel_dim}, ent), g_t = empty_f32({t.num_ent, t.dim}, ent);
  check(kge_bce_dist_bwd(&t, (int)direction, ai, pi, n, l.rowptr.data_ptr<int64_t>(), l.col.data_ptr<int64_t>(),
                         (float)offset, l.g, (float)g_scalar, g_a.data_ptr<float>(), g_p.data_ptr<float>(),
                         g_t.data_ptr<float>(), ce_dist_ws(workspace, workspace_bytes), workspace_bytes, stream_of(ent)),
        "kge_bce_dist_bwd");
  return {g_a, g_p, g_t};
}

// ---- the KvsAll losses of ComplEx / DistMult on FLOAT32 tables (kge_kl_f32_* / kge_bce_f32_*): the signatures of the
// distance twins above, plus label_bias in the kl backward; workspace: kge_multilabel_f32_workspace_bytes.
int64_t multilabel_f32_workspace_bytes(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm,
                                       int64_t n, int64_t chunk_cols) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, 0);
  return kge_multilabel_f32_workspace_bytes(&t, n, chunk_cols);
}

std::vector<at::Tensor> kl_f32_fwd(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm,
                                   int64_t direction, const at::Tensor& a, const at::Tensor& p, const at::Tensor& rowptr,
                                   const at::Tensor& col, const c10::optional<at::Tensor>& label_weight,
                                   const at::Tensor& workspace, int64_t workspace_bytes) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, 0);
  std::vector<at::Tensor> keep;
  int64_t n = -1;
  const kge_index ai = index_of(a, ent, keep, &n), pi = index_of(p, ent, keep, &n);
  const DistLabels l = dist_labels(ent, n, rowptr, col, label_weight, c10::nullopt);
  at::Tensor loss_rows = empty_f32({n}, ent), lse = empty_f32({n}, ent);
  check(kge_kl_f32_fwd(&t, (int)direction, ai, pi, n, l.rowptr.data_ptr<int64_t>(), l.col.data_ptr<int64_t>(), l.w,
                       loss_rows.data_ptr<float>(), lse.data_ptr<float>(), ce_dist_ws(workspace, workspace_bytes),
                       workspace_bytes, stream_of(ent)),
        "kge_kl_f32_fwd");
  return {loss_rows, lse};
}

std::vector<at::Tensor> kl_f32_bwd(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm,
                                   int64_t direction, const at::Tensor& a, const at::Tensor& p, const at::Tensor& rowptr,
                                   const at::Tensor& col, const c10::optional<at::Tensor>& label_weight,
                                   const c10::optional<at::Tensor>& label_bias, const at::Tensor& lse,
                                   const c10::optional<at::Tensor>& g_rows, double g_scalar, const at::Tensor& workspace,
                                   int64_t workspace_bytes) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, 0);
  std::vector<at::Tensor> keep;
  int64_t n = -1;
  const kge_index ai = index_of(a, ent, keep, &n), pi = index_of(p, ent, keep, &n);
  const DistLabels l = dist_labels(ent, n, rowptr, col, label_weight, g_rows);
  const at::Tensor lse_c = lse.to(at::kFloat).contiguous();
  TORCH_CHECK_VALUE(lse_c.numel() == n, "kge_amd: lse must have one entry per row");
  at::Tensor lb;
  if (label_bias.has_value() && label_bias->defined()) {
    lb = label_bias->to(at::kFloat).contiguous();
    TORCH_CHECK_VALUE(lb.numel() == n, "kge_amd: label_bias must have one entry per row");
  }
  at::Tensor g_a = empty_f32({n, t.dim}, ent), g_p = empty_f32({n, t.rel_dim}, ent), g_t = empty_f32({t.num_ent, t.dim}, ent);
  check(kge_kl_f32_bwd(&t, (int)direction, ai, pi, n, l.rowptr.data_ptr<int64_t>(), l.col.data_ptr<int64_t>(), l.w,
                       lb.defined() ? lb.data_ptr<float>() : nullptr, lse_c.data_ptr<float>(), l.g, (float)g_scalar,
                       g_a.data_ptr<float>(), g_p.data_ptr<float>(), g_t.data_ptr<float>(),
                       ce_dist_ws(workspace, workspace_bytes), workspace_bytes, stream_of(ent)),
        "kge_kl_f32_bwd");
  return {g_a, g_p, g_t};
}

at::Tensor bce_f32_fwd(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm, int64_t direction,
                       const at::Tensor& a, const at::Tensor& p, const at::Tensor& rowptr, const at::Tensor& col,
                       double offset, const at::Tensor& workspace, int64_t workspace_bytes) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, 0);
  std::vector<at::Tensor> keep;
  int64_t n = -1;
  const kge_index ai = index_of(a, ent, keep, &n), pi = index_of(p, ent, keep, &n);
  const DistLabels l = dist_labels(ent, n, rowptr, col, c10::nullopt, c10::nullopt);
  at::Tensor loss_rows = empty_f32({n}, ent);
  check(kge_bce_f32_fwd(&t, (int)direction, ai, pi, n, l.rowptr.data_ptr<int64_t>(), l.col.data_ptr<int64_t>(),
                        (float)offset, loss_rows.data_ptr<float>(), ce_dist_ws(workspace, workspace_bytes),
                        workspace_bytes, stream_of(ent)),
        "kge_bce_f32_fwd");
  return loss_rows;
}

std::vector<at::Tensor> bce_f32_bwd(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm,
                                    int64_t direction, const at::Tensor& a, const at::Tensor& p, const at::Tensor& rowptr,
                                    const at::Tensor& col, double offset, const c10::optional<at::Tensor>& g_rows,
                                    double g_scalar, const at::Tensor& workspace, int64_t workspace_bytes) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, 0);
  std::vector<at::Tensor> keep;
  int64_t n = -1;
  const kge_index ai = index_of(a, ent, keep, &n), pi = index_of(p, ent, keep, &n);
  const DistLabels l = dist_labels(ent, n, rowptr, col, c10::nullopt, g_rows);
  at::Tensor g_a = empty_f32({n, t.dim}, ent), g_p = empty_f32({n, t.rel_dim}, ent), g_t = empty_f32({t.num_ent, t.dim}, ent);
  check(kge_bce_f32_bwd(&t, (int)direction, ai, pi, n, l.rowptr.data_ptr<int64_t>(), l.col.data_ptr<int64_t>(),
                        (float)offset, l.g, (float)g_scalar, g_a.data_ptr<float>(), g_p.data_ptr<float>(),
                        g_t.data_ptr<float>(), ce_dist_ws(workspace, workspace_bytes), workspace_bytes, stream_of(ent)),
        "kge_bce_f32_bwd");
  return {g_a, g_p, g_t};
}

// ---- every negative-sampling loss over one slot's scores (kge_ns_loss): pos [n] of any stride, neg [n, K] with unit
// inner stride (a slice of a wider matrix is fine).  -> (loss_rows [n], g_pos [n], g_neg [n, K]); the gradients are
// undefined tensors (None in Python) without want_grad.
std::vector<at::Tensor> ns_loss_parts(const at::Tensor& pos, const at::Tensor& neg, int64_t kind, double arg,
                                      double temperature, bool want_grad) {
  TORCH_CHECK(pos.is_cuda() && neg.is_cuda() && pos.get_device() == neg.get_device(),
              "kge_amd: ns_loss takes GPU tensors on one device (no CPU path)");
  TORCH_CHECK_VALUE(pos.scalar_type() == at::kFloat && neg.scalar_type() == at::kFloat && pos.dim() == 1 && neg.dim() == 2 &&
                        neg.size(0) == pos.size(0) && neg.size(1) >= 1 && (neg.size(1) == 1 || neg.stride(1) == 1),
                    "kge_amd: ns_loss takes float32 pos [n] and neg [n, K >= 1] with unit inner stride");
  const int64_t n = neg.size(0), K = neg.size(1);
  TORCH_CHECK_VALUE(n <= 1 || (pos.stride(0) >= 0 && neg.stride(0) >= K), "kge_amd: ns_loss: overlapping or reversed rows");
  at::Tensor rows = empty_f32({n}, neg), g_pos, g_neg;
  if (want_grad) {
    g_pos = empty_f32({n}, neg);
    g_neg = empty_f32({n, K}, neg);
  }
  check(kge_ns_loss(pos.data_ptr<float>(), n > 1 ? pos.stride(0) : 1, neg.data_ptr<float>(), n > 1 ? neg.stride(0) : K, n, K,
                    (int)kind, (float)arg, (float)temperature, rows.data_ptr<float>(),
                    want_grad ? g_pos.data_ptr<float>() : nullptr, 1, want_grad ? g_neg.data_ptr<float>() : nullptr, K,
                    stream_of(neg)),
        "kge_ns_loss");
  return {rows, g_pos, g_neg};
}

// ---- one slot's negative samples drawn on the device (kge_neg_sample): -> (out int64 [n, K], stats int32 [n, 2] or an
// undefined tensor).  alias = (prob float32 [vocab], idx int64 [vocab]) or neither; index = (sorted_keys, starts, values)
// int64 with the key columns a, b [n], or none of them (unfiltered).  `like` names the device.
std::vector<at::Tensor> neg_sample(const at::Tensor& like, int64_t n, int64_t K, int64_t vocab, int64_t slot, uint64_t seed,
                                   uint64_t call, const c10::optional<at::Tensor>& alias_prob,
                                   const c10::optional<at::Tensor>& alias_idx, const c10::optional<at::Tensor>& sorted_keys,
                                   const c10::optional<at::Tensor>& starts, const c10::optional<at::Tensor>& values,
                                   const c10::optional<at::Tensor>& a, const c10::optional<at::Tensor>& b, int64_t mult,
                                   bool want_stats) {
  TORCH_CHECK(like.is_cuda(), "kge_amd: neg_sample draws on a GPU (no CPU path)");
  TORCH_CHECK_VALUE(n >= 0 && K >= 0, "kge_amd: neg_sample: negative shape");
  const auto on_dev = [&](const c10::optional<at::Tensor>& t, at::ScalarType ty, const char* what) -> const void* {
    if (!t.has_value() || !t->defined()) return nullptr;
    TORCH_CHECK(t->is_cuda() && t->get_device() == like.get_device(), "kge_amd: neg_sample: ", what, " on ", t->device());
    TORCH_CHECK_VALUE(t->scalar_type() == ty && t->is_contiguous(), "kge_amd: neg_sample: ", what, ": dtype / layout");
    return t->data_ptr();
  };
  const float* ap = (const float*)on_dev(alias_prob, at::kFloat, "alias_prob");
  const int64_t* ai = (const int64_t*)on_dev(alias_idx, at::kLong, "alias_idx");
  TORCH_CHECK_VALUE(!ap || (ai && alias_prob->numel() == vocab && alias_idx->numel() == vocab),
                    "kge_amd: neg_sample: the alias tables are [vocab] each");
  const int64_t* keys = (const int64_t*)on_dev(sorted_keys, at::kLong, "sorted_keys");
  const int64_t* st = (const int64_t*)on_dev(starts, at::kLong, "starts");
  const int64_t* vals = (const int64_t*)on_dev(values, at::kLong, "values");
  std::vector<at::Tensor> keep;
  kge_index ia{nullptr, KGE_I64, 0, 1}, ib = ia;
  int64_t num_keys = 0;
  if (keys) {
    TORCH_CHECK_VALUE(st && vals && starts->numel() == sorted_keys->numel() + 1, "kge_amd: neg_sample: starts is [num_keys + 1]");
    num_keys = sorted_keys->numel();
    int64_t len = n;
    ia = index_of(a, like, keep, &len);
    ib = index_of(b, like, keep, &len);
  }
  at::Tensor out, stats;
  try {
    out = at::empty({n, K}, like.options().dtype(at::kLong));
    if (want_stats) stats = at::empty({n, 2}, like.options().dtype(at::kInt));
  } catch (const c10::OutOfMemoryError& e) {
    TORCH_CHECK(false, "CUDA out of memory (kge_amd, ROCm: ", e.what_without_backtrace(), ")");
  }
  check(kge_neg_sample(n, K, vocab, (int)slot, seed, call, ap, ai, keys, num_keys, st, vals, ia, ib, mult,
                       out.data_ptr<int64_t>(), K, want_stats ? stats.data_ptr<int32_t>() : nullptr, stream_of(like)),
        "kge_neg_sample");
  return {out, stats};
}

// ---- a KvsAll batch collated on the device (kge_kvsall_collate; train_KvsAll.py:118-201 + the per-type CSR cut).
// keys / offsets / values: the index arrays of each query type (int64, on the GPU), lasts / target_cols per type; caps
// empty (no typed form) or (rows_cap, lab_cap) per type, flat.  -> [queries, query_type, label_coords, triples] if
// want_batch, then (ids, rowptr, col, weight, rows) per type if caps, then counts int64 [num_types, 3].
std::vector<at::Tensor> kvsall_collate(const at::Tensor& examples, const std::vector<at::Tensor>& keys,
                                       const std::vector<at::Tensor>& offsets, const std::vector<at::Tensor>& values,
                                       const std::vector<int64_t>& lasts, const std::vector<int64_t>& target_cols,
                                       int64_t nnz, bool want_batch, const std::vector<int64_t>& caps, double weight) {
  TORCH_CHECK(examples.is_cuda(), "kge_amd: kvsall_collate builds the batch on a GPU (no CPU path)");
  const size_t T = keys.size();
  TORCH_CHECK_VALUE(T >= 1 && T <= 3 && offsets.size() == T && values.size() == T && lasts.size() == T &&
                        target_cols.size() == T && (caps.empty() || caps.size() == 2 * T),
                    "kge_amd: kvsall_collate: 1 to 3 query types, every list one entry per type");
  TORCH_CHECK_VALUE(examples.scalar_type() == at::kLong && examples.dim() == 1 && examples.is_contiguous() && nnz >= 0,
                    "kge_amd: kvsall_collate: examples is a contiguous int64 vector");
  const auto ptr = [&](const at::Tensor& t, const char* what) -> const int64_t* {
    TORCH_CHECK(t.is_cuda() && t.get_device() == examples.get_device(), "kge_amd: kvsall_collate: ", what, " on ", t.device());
    TORCH_CHECK_VALUE(t.scalar_type() == at::kLong && t.is_contiguous(), "kge_amd: kvsall_collate: ", what, ": dtype / layout");
    return t.data_ptr<int64_t>();
  };
  kge_kvsall_index ix[3];
  kge_kvsall_typed ty[3];
  const int64_t n = examples.numel();
  const auto i64 = examples.options();
  std::vector<at::Tensor> res;
  at::Tensor ws, counts;
  try {
    if (want_batch) {
      res.push_back(at::empty({n, 2}, i64));
      res.push_back(at::empty({n}, i64));
      res.push_back(at::empty({nnz, 2}, i64.dtype(at::kInt)));
      res.push_back(at::empty({nnz, 3}, i64));
    }
    for (size_t t = 0; t < T; ++t) {
      int64_t prev = t ? lasts[t - 1] : 0;
      TORCH_CHECK_VALUE(lasts[t] >= prev && keys[t].numel() == 2 * (lasts[t] - prev) &&
                            offsets[t].numel() == lasts[t] - prev + 1,
                        "kge_amd: kvsall_collate: keys [M, 2] and offsets [M + 1] with M = the type's examples");
      ix[t] = kge_kvsall_index{ptr(keys[t], "keys"), ptr(offsets[t], "offsets"), ptr(values[t], "values"), lasts[t],
                               (int32_t)target_cols[t], 0};
      if (!caps.empty()) {
        const int64_t rc = caps[2 * t], lc = caps[2 * t + 1];
        TORCH_CHECK_VALUE(rc >= 0 && lc >= 0, "kge_amd: kvsall_collate: negative capacity");
        at::Tensor ids = at::empty({rc, 2}, i64), rp = at::empty({rc + 1}, i64), col = at::empty({lc}, i64);
        at::Tensor w = at::empty({rc}, i64.dtype(at::kFloat)), rows = at::empty({rc}, i64);
        ty[t] = kge_kvsall_typed{ids.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), col.data_ptr<int64_t>(),
                                 w.data_ptr<float>(), rows.data_ptr<int64_t>(), rc, lc};
        res.insert(res.end(), {ids, rp, col, w, rows});
      }
    }
    counts = at::empty({(int64_t)T, 3}, i64);
    ws = at::empty({kge_kvsall_collate_workspace_bytes(n) / 8}, i64);
  } catch (const c10::OutOfMemoryError& e) {
    TORCH_CHECK(false, "CUDA out of memory (kge_amd, ROCm: ", e.what_without_backtrace(), ")");
  }
  check(kge_kvsall_collate(ix, (int)T, examples.data_ptr<int64_t>(), n, nnz,
                           want_batch ? res[0].data_ptr<int64_t>() : nullptr,
                           want_batch ? res[1].data_ptr<int64_t>() : nullptr,
                           want_batch ? res[2].data_ptr<int32_t>() : nullptr,
                           want_batch ? res[3].data_ptr<int64_t>() : nullptr, caps.empty() ? nullptr : ty, (float)weight,
                           counts.data_ptr<int64_t>(), n ? ws.data_ptr() : nullptr, ws.numel() * 8, stream_of(examples)),
        "kge_kvsall_collate");
  res.push_back(counts);
  return res;
}

// ---- filtered top-k prediction (kge_topk; direction: 1 = sp_, 2 = _po): (values [n, k] float32, ids [n, k] int64).
// filters: 3 tensors per set (begin [n], end [n], col [nnz], int64); workspace: the caller's (engine.py caches one per
// device and stream), at least topk_workspace_bytes(...) bytes.
int64_t topk_workspace_bytes(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm, int64_t flags,
                             int64_t n, int64_t m, int64_t k, int64_t num_filters) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, flags);
  return kge_topk_workspace_bytes(&t, n, m, (int)k, (int)num_filters);
}

std::vector<at::Tensor> topk(const at::Tensor& ent, const at::Tensor& rel, int64_t scorer, double l_norm, int64_t flags,
                             int64_t direction, const at::Tensor& a, const at::Tensor& p, int64_t k,
                             const std::vector<at::Tensor>& filters, const c10::optional<at::Tensor>& keep,
                             int64_t col_begin, int64_t m, const c10::optional<at::Tensor>& workspace) {
  const kge_tables t = tables_of(ent, rel, scorer, l_norm, flags);
  TORCH_CHECK_VALUE(k >= 1 && k <= KGE_TOPK_MAX, "kge_amd: topk: k must be in [1, ", (int)KGE_TOPK_MAX, "], got ", k);
  TORCH_CHECK_VALUE(filters.size() % 3 == 0 && filters.size() <= 6, "kge_amd: topk: at most two (begin, end, col) filter sets");
  std::vector<at::Tensor> keep_alive;
  int64_t n = -1;
  const kge_index ai = index_of(a, ent, keep_alive, &n), pi = index_of(p, ent, keep_alive, &n);
  const kge_index ki = index_of(keep, ent, keep_alive, &n);
  const int K = (int)(filters.size() / 3);
  const int64_t* fb[2] = {nullptr, nullptr};
  const int64_t* fe[2] = {nullptr, nullptr};
  const int64_t* fc[2] = {nullptr, nullptr};
  for (int f = 0; f < K; ++f) {
    for (int j = 0; j < 3; ++j) {
      const at::Tensor& x = filters[3 * f + j];
      TORCH_CHECK_VALUE(x.is_cuda() && x.get_device() == ent.get_device() && x.scalar_type() == at::kLong &&
                            x.is_contiguous() && (j == 2 || x.numel() == n),
                        "kge_amd: topk: a filter set is (begin [n], end [n], col [nnz]), contiguous int64 on the tables' GPU");
    }
    fb[f] = filters[3 * f].data_ptr<int64_t>();
    fe[f] = filters[3 * f + 1].data_ptr<int64_t>();
    fc[f] = filters[3 * f + 2].data_ptr<int64_t>();
  }
  void* ws = nullptr;
  int64_t wsb = 0;
  if (workspace.has_value() && workspace->defined()) {
    TORCH_CHECK(workspace->is_cuda() && workspace->is_contiguous(), "kge_amd: workspace must be a contiguous GPU tensor");
    ws = workspace->data_ptr();
    wsb = workspace->numel() * workspace->element_size();
  }
  at::Tensor val = empty_f32({n, k}, ent);
  at::Tensor idx;
  try {
    idx = at::empty({n, k}, ent.options().dtype(at::kLong));
  } catch (const c10::OutOfMemoryError& e) {
    TORCH_CHECK(false, "CUDA out of memory (kge_amd, ROCm: ", e.what_without_backtrace(), ")");
  }
  check(kge_topk(&t, (int)direction, ai, pi, n, col_begin, m, (int)k, K, fb, fe, fc, ki, val.data_ptr<float>(),
                 idx.data_ptr<int64_t>(), k, ws, wsb, stream_of(ent)),
        "kge_topk");
  return {val, idx};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.doc() = "kge_amd: PyTorch-ROCm binding of libkge_amd.so (include/kge_amd.h)";
  mod.def("abi_version", []() { return kge_abi_version(); });
  mod.def("score_spo", &score_spo, "KgeModel.score_spo: [n] scores");
  mod.def("score_pairs", &score_pairs, "KgeModel.score_sp / score_po / score_sp_po: [n, m] / [n, 2 m] scores");
  mod.def("score_so", &score_so, "KgeModel.score_so: [n, m] scores of (s[i], rels[j], o[i]); rels None = all relations");
  mod.def("score_so_bwd_accum", &score_so_bwd_accum, "its backward into the dense table gradients; False: declined");
  mod.def("queries_bytes", &queries_bytes);
  mod.def("build_queries_group", &build_queries_group);
  mod.def("score_queries_group", &score_queries_group);
  mod.def("ce_dist_workspace_bytes", &ce_dist_workspace_bytes);
  mod.def("ce_dist_fwd", &ce_dist_fwd, "1vsAll cross entropy of TransE / RotatE without a score matrix: (loss_rows, lse)");
  mod.def("ce_dist_bwd", &ce_dist_bwd, "its backward: (g_a, g_p, g_entities)");
  mod.def("ce_f32_workspace_bytes", &ce_f32_workspace_bytes);
  mod.def("ce_f32_fwd", &ce_f32_fwd, "1vsAll cross entropy of float32 ComplEx / DistMult without a score matrix: (loss_rows, lse)");
  mod.def("ce_f32_bwd", &ce_f32_bwd, "its backward: (g_a, g_p, g_entities)");
  mod.def("multilabel_dist_workspace_bytes", &multilabel_dist_workspace_bytes);
  mod.def("kl_dist_fwd", &kl_dist_fwd, "KvsAll kl loss of TransE / RotatE without a score matrix: (loss_rows, lse)");
  mod.def("kl_dist_bwd", &kl_dist_bwd, "its backward: (g_a, g_p, g_entities)");
  mod.def("bce_dist_fwd", &bce_dist_fwd, "KvsAll bce loss of TransE / RotatE without a score matrix: loss_rows");
  mod.def("bce_dist_bwd", &bce_dist_bwd, "its backward: (g_a, g_p, g_entities)");
  mod.def("multilabel_f32_workspace_bytes", &multilabel_f32_workspace_bytes);
  mod.def("kl_f32_fwd", &kl_f32_fwd, "KvsAll kl loss of float32 ComplEx / DistMult without a score matrix: (loss_rows, lse)");
  mod.def("kl_f32_bwd", &kl_f32_bwd, "its backward (label_bias: the uniform term of smoothed labels): (g_a, g_p, g_entities)");
  mod.def("bce_f32_fwd", &bce_f32_fwd, "KvsAll bce loss of float32 ComplEx / DistMult without a score matrix: loss_rows");
  mod.def("bce_f32_bwd", &bce_f32_bwd, "its backward: (g_a, g_p, g_entities)");
  mod.def("ns_loss_parts", &ns_loss_parts,
          "negative-sampling loss of one slot from (pos [n], neg [n, K]): (loss_rows, g_pos, g_neg)");
  mod.def("neg_sample", &neg_sample, "one slot's negative samples drawn, filtered and redrawn on the device: (out, stats)");
  mod.def("topk_workspace_bytes", &topk_workspace_bytes);
  mod.def("topk", &topk, "the k best unfiltered entities per query without a score matrix: (values [n, k], ids [n, k])");
  mod.def("kvsall_collate", &kvsall_collate,
          "a KvsAll batch from its example numbers, on the device: the collate dictionary and / or the per-type CSR");
}
