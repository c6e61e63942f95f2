// fdnn_lazy_entries.cpp -- lazy output for ENTRIES: only some (row, node) pairs of the output layer are scored.  The callers
// name them as active-node lists (run_lists), one node set for a row range (run_set) or one set per segment (run_sets); a
// call of any of them is the same five steps, and run_entries below is their one home: the argument checks, the output
// layer's view, e = exp(z) of the entries into probs by the caller's score step, the finish pass (fdnn_lists.hip: every
// total and scale), the error check.  entries_to_host is the one host form.  Nothing of the masked output path runs.
#include <algorithm>
#include <climits>
#include <string>
#include <vector>

#include "fdnn_internal.hpp"

namespace fdnn {

int lazy_state(const fdnn_ctx *c) {
  return c->last < 0 ? fail(FDNN_E_STATE, "lazy output requested before the hidden layers were computed") : FDNN_OK;
}

// What the list kernels and the set kernel read of the output layer (a context whose hidden layers have run).
static ListsParams output_layer_params(const fdnn_ctx *c, int first) {
  const fdnn_model *m = c->m;
  const BlobHeader &h = m->hm.hdr;
  const QLayerDesc &d = h.q[h.n_q - 1];
  const uint8_t *B = m->d_blob;
  ListsParams g{};
  g.w = reinterpret_cast<const int8_t *>(B + d.off_w);
  g.a = c->d_act[c->last] + size_t(first) * c->act_ld;
  g.bias = reinterpret_cast<const float *>(B + d.off_bias);
  g.wsum = reinterpret_cast<const int32_t *>(B + d.off_wsum);
  if (d.n_fix > 0) {
    g.fix_off = m->d_lfix_off;
    g.fix_pairs = m->d_lfix_pairs;
  }
  g.rows = d.rows;
  g.K = d.cols_pad - kRowSkew;
  g.ldw = d.cols_pad;
  g.lda = c->act_ld;
  g.coef = d.coef;
  g.rcp_coef = d.rcp_coef;
  g.fastdiv = d.fastdiv_ok;
  return g;
}

// The same view for the kernels over the set tile; what they read besides the layer (nodes, probs, acc, count, len, plan) is
// the caller's to fill in.
static SetParams set_params(const ListsParams &g) {
  SetParams p{};
  p.w = g.w, p.a = g.a, p.bias = g.bias, p.wsum = g.wsum, p.fix_off = g.fix_off, p.fix_pairs = g.fix_pairs;
  p.rows = g.rows, p.K = g.K, p.ldw = g.ldw, p.lda = g.lda;
  p.coef = g.coef, p.rcp_coef = g.rcp_coef, p.fastdiv = g.fastdiv;
  return p;
}

UnionParams union_params(const lunion::Layout &l, int32_t *b, const ListsCall &lc, int rows, int group_tiles) {
  return {lc.d_row_ptr, lc.d_nodes, lc.d_probs, lc.d_acc, b + l.u_nodes, b + l.pos, b + l.u_len, b + l.work, b + l.counter,
          rows, lc.count, lc.nnz, group_tiles, int(l.bound)};
}

// fdnn_debug_set_kernel: the default rule (mode 0) is mode 1's, the MFMA kernels wherever their shape applies
static bool set_tile_serves(const ListsParams &g) { return set_kernel_mode() != 2 && set::shape_applies(g.K, g.rows, g.ldw, g.lda); }

// One lazy-entries call on rows [first, first + count) with nnz entries.  The finish pass's rows are the caller's device
// row pointer (by_row_ptr), a uniform row_len, or a row pointer the score step leaves in its ListsParams.
struct EntriesCall {
  int first = 0, count = 0, nnz = 0;
  bool by_row_ptr = false;
  const int32_t *d_row_ptr = nullptr;
  int row_len = 0;
  const int32_t *d_nodes = nullptr;  // (only looked at for being there: the score step reads them)
  float *d_probs = nullptr;
  float *d_inactive = nullptr;
  int32_t *d_acc = nullptr;
  const char *bad = nullptr;  // the caller's own argument check has failed: its text, reported behind the row range's
};

// score(g) enqueues on s whatever writes e = exp(z) of every entry to g.probs (and g.acc), under its own FDNN_PROF_OUTPUT
// scope, and returns a status; g is the layer's view with the call's results, count and nnz.
template <class Score>
static int run_entries(fdnn_ctx *c, const EntriesCall &ec, hipStream_t s, Score &&score) {
  if (int rc = lazy_state(c)) return rc;
  if (ec.first < 0 || ec.count < 0 || ec.first + ec.count > c->n) return fail(FDNN_E_ARG, "frame range outside the context");
  if (ec.bad) return fail(FDNN_E_ARG, ec.bad);
  if (ec.count == 0) return FDNN_OK;
  if ((ec.by_row_ptr && !ec.d_row_ptr) || !ec.d_inactive || (ec.nnz > 0 && (!ec.d_nodes || !ec.d_probs)))
    return fail(FDNN_E_ARG, ec.by_row_ptr ? "null list buffer" : "null set buffer");
  ListsParams g = output_layer_params(c, ec.first);
  g.row_ptr = ec.d_row_ptr;
  g.probs = ec.d_probs;
  g.inactive = ec.d_inactive;
  g.acc = ec.d_acc;
  g.count = ec.count;
  g.nnz = ec.nnz;
  if (int rc = score(g)) return rc;
  if (!g.row_ptr) g.row_len = ec.row_len;  // the finish kernel's uniform rows: r * len .. (r + 1) * len
  {
    ProfScope ps(c->m, s, FDNN_PROF_NORMALIZE);
    launch_lists_finish(g, s);
  }
  HIP_TRY(hipGetLastError());
  return FDNN_OK;
}

// The dot-product kernels over the lists in g
static int score_lists(fdnn_ctx *c, ListsParams &g, hipStream_t s) {
  g.epg = lists_entries_per_group(g.nnz, device_cus(c->m->device));
  ProfScope ps(c->m, s, FDNN_PROF_OUTPUT);
  launch_lists_score(g, s);
  return FDNN_OK;
}

// The set forms' fallback: `expand` writes the call's sets out as lists -- nodes into d_snodes, under the row pointer in
// d_srow -- and the list kernels score them: the same bytes by construction.
template <class Expand>
static int score_as_lists(fdnn_ctx *c, ListsParams &g, hipStream_t s, Expand &&expand) {
  HIP_TRY(c->d_snodes.reserve(size_t(g.nnz)));
  expand();
  g.row_ptr = c->d_srow;
  g.nodes = c->d_snodes;
  return score_lists(c, g, s);
}

// LazyOutputActivations for the listed nodes only (fdnn_lists.hip): the score kernel over the flat entry array, then one
// wave per row for the total and the scale.
int run_lists(fdnn_ctx *c, const ListsCall &lc, hipStream_t s) {
  fdnn_model *m = c->m;
  const EntriesCall ec{.first = lc.first, .count = lc.count, .nnz = lc.nnz, .by_row_ptr = true, .d_row_ptr = lc.d_row_ptr, .d_nodes = lc.d_nodes,
                       .d_probs = lc.d_probs, .d_inactive = lc.d_inactive, .d_acc = lc.d_acc, .bad = lc.nnz < 0 ? "negative entry count" : nullptr};
  return run_entries(c, ec, s, [&](ListsParams &g) -> int {
    g.nodes = lc.d_nodes;
    // fdnn_model_set_lists_union: the entries' e from the set kernels' tile over the union of every 32 g rows' lists
    // (fdnn_lists_union.hip) where its shape applies -- the same bytes; else, and with the switch off, the dot-product kernels
    const int group_tiles = m->lists_union;
    const bool by_union = group_tiles > 0 && lunion::shape_applies(g.K, g.rows, g.ldw, g.lda);
    if (group_tiles > 0 && !by_union) lists_union_note_fallback();
    if (!by_union) return score_lists(c, g, s);
    if (lc.nnz == 0) return FDNN_OK;
    const lunion::Layout l = lunion::layout(lc.nnz, lc.count, group_tiles);
    if (l.bound > INT32_MAX / 2) return fail(FDNN_E_ARG, "too many entries for one list call");
    // (a buffer that is too small is freed and allocated anew, which waits for the device: earlier calls have finished)
    HIP_TRY(c->d_union.reserve(l.words));
    const UnionParams u = union_params(l, c->d_union.p, lc, g.rows, group_tiles);
    ProfScope ps(m, s, FDNN_PROF_OUTPUT);
    HIP_TRY(launch_lists_union_build(u, l.n_groups, s));
    launch_lists_union_score(set_params(g), u, device_cus(m->device), s);
    return FDNN_OK;
  });
}

// LazyOutputActivations for ONE node set shared by rows [first, first + count) (fdnn_set.hip): e = exp(z) of the gathered
// rows on the int8 MFMA, then the list path's finish kernel with the uniform row stride len.  Where the MFMA kernel's shape
// does not apply (fdnn_set.hpp: shape_applies) the list kernels serve the call over lists synthesized from the set.
int run_set(fdnn_ctx *c, const SetCall &sc, hipStream_t s) {
  fdnn_model *m = c->m;
  const long long nnz = static_cast<long long>(sc.count) * sc.len;
  const char *bad = nullptr;
  if (sc.len < 0 || sc.len > m->hm.hdr.out_dim) bad = "a node set has 0 .. output_dim nodes";
  else if (nnz > INT32_MAX) bad = "count x len must fit an int32";
  const EntriesCall ec{.first = sc.first, .count = sc.count, .nnz = int(nnz), .row_len = sc.len, .d_nodes = sc.d_nodes, .d_probs = sc.d_probs,
                       .d_inactive = sc.d_inactive, .d_acc = sc.d_acc, .bad = bad};
  return run_entries(c, ec, s, [&](ListsParams &g) -> int {
    if (sc.len == 0) return FDNN_OK;
    if (set_tile_serves(g)) {
      SetParams p = set_params(g);
      p.nodes = sc.d_nodes, p.probs = sc.d_probs, p.acc = sc.d_acc, p.count = sc.count, p.len = sc.len;
      p.plan = set::plan(sc.count, sc.len, device_cus(m->device));
      ProfScope ps(m, s, FDNN_PROF_OUTPUT);
      launch_set_score(p, s);
      return FDNN_OK;
    }
    // (a buffer that is too small is freed and allocated anew, which waits for the device: earlier calls have finished)
    HIP_TRY(c->d_srow.reserve(size_t(sc.count) + 1));
    return score_as_lists(c, g, s, [&] { launch_set_expand(sc.d_nodes, sc.len, sc.count, c->d_srow, c->d_snodes, s); });
  });
}

// LazyOutputActivations with one node set per segment (fdnn_sets.hip): the set kernel's tile on every segment, at most
// sets::kMaxSegs segments per launch, then the list path's finish kernel over the row pointer of the ragged blocks.  Where
// the MFMA kernel's shape does not apply the list kernels serve the call over the sets written out as lists.
int run_sets(fdnn_ctx *c, const SetsCall &sc, hipStream_t s) {
  fdnn_model *m = c->m;
  if (int rc = lazy_state(c)) return rc;
  if (!sc.segs) return fail(FDNN_E_ARG, "null argument");
  const std::vector<sets::Seg> &segs = *sc.segs;
  long long nnz = 0;
  int count = 0;
  for (size_t i = 0; i < segs.size(); ++i) {
    const sets::Seg &g = segs[i];
    if (g.rows < 0 || g.row0 != count) return fail(FDNN_E_ARG, "segment " + std::to_string(i) + ": rows must follow the segment before");
    if (g.len < 0 || g.len > m->hm.hdr.out_dim || g.set_off < 0)
      return fail(FDNN_E_ARG, "segment " + std::to_string(i) + ": a node set has 0 .. output_dim nodes");
    if (g.out_off != nnz) return fail(FDNN_E_ARG, "segment " + std::to_string(i) + ": blocks must follow each other");
    count += g.rows;
    nnz += static_cast<long long>(g.rows) * g.len;
    if (nnz > INT32_MAX) return fail(FDNN_E_ARG, "segment " + std::to_string(i) + ": the sum of rows x len must fit an int32");
  }
  const EntriesCall ec{.first = sc.first, .count = count, .nnz = int(nnz), .d_nodes = sc.d_nodes, .d_probs = sc.d_probs,
                       .d_inactive = sc.d_inactive, .d_acc = sc.d_acc};
  return run_entries(c, ec, s, [&](ListsParams &g) -> int {
    const bool mfma = set_tile_serves(g);
    // the finish pass's row pointer [count + 1] and, for the fallback, where each row's set begins [count], side by side in
    // the staging buffer: written on the device from the launch tables, so an enqueued call leaves no host memory behind.
    // (A buffer that is too small is freed and allocated anew, which waits for the device: earlier calls have finished.)
    HIP_TRY(c->d_srow.reserve(size_t(2) * size_t(count) + 1));
    int32_t *const d_row_set = mfma ? nullptr : c->d_srow.p + count + 1;
    const std::vector<sets::Launch> launches = sets::plan(segs, device_cus(m->device));
    for (size_t i = 0; i < launches.size(); ++i)
      launch_sets_rows(launches[i], c->d_srow, d_row_set, i + 1 == launches.size() ? count : -1, int(nnz), s);
    g.row_ptr = c->d_srow;
    if (nnz == 0) return FDNN_OK;
    if (!mfma) return score_as_lists(c, g, s, [&] { launch_sets_expand(sc.d_nodes, c->d_srow, d_row_set, count, c->d_snodes, s); });
    SetParams p = set_params(g);
    p.nodes = sc.d_nodes, p.probs = sc.d_probs, p.acc = sc.d_acc;
    ProfScope ps(m, s, FDNN_PROF_OUTPUT);
    for (const sets::Launch &l : launches) launch_sets_score(p, l, s);
    return FDNN_OK;
  });
}

int entries_to_host(fdnn_ctx *c, const HostEntries &h, hipStream_t s) {
  const size_t count = size_t(h.count);
  size_t nnz = h.row_ptr ? size_t(h.row_ptr[count]) : count * size_t(h.len);
  if (h.segs) {
    nnz = 0;
    for (const sets::Seg &g : *h.segs) nnz += size_t(g.rows) * size_t(g.len);
  }
  if (nnz > size_t(INT32_MAX)) return fail(FDNN_E_ARG, "the entries of one call must fit an int32");  // (the callers have checked)
  // (a buffer that is too small is freed and allocated anew: the context's earlier list calls have been synchronised)
  if (h.row_ptr) HIP_TRY(c->d_lrow.reserve(count + 1));
  HIP_TRY(c->d_linact.reserve(std::max<size_t>(count, 1)));
  HIP_TRY(c->d_lnodes.reserve(std::max<size_t>(size_t(h.n_nodes), 1)));
  HIP_TRY(c->d_lprobs.reserve(std::max<size_t>(nnz, 1)));
  DevBuf<int32_t> d_acc;
  if (h.acc) HIP_TRY(d_acc.reserve(std::max<size_t>(nnz, 1)));
  if (h.row_ptr) HIP_TRY(hipMemcpyAsync(c->d_lrow, h.row_ptr, sizeof(int32_t) * (count + 1), hipMemcpyHostToDevice, s));
  if (h.n_nodes > 0) HIP_TRY(hipMemcpyAsync(c->d_lnodes, h.nodes, sizeof(int32_t) * size_t(h.n_nodes), hipMemcpyHostToDevice, s));
  int32_t *const acc = h.acc ? d_acc.p : nullptr;
  int rc;
  if (h.row_ptr) {
    rc = run_lists(c, {h.first, h.count, c->d_lrow, c->d_lnodes, int(nnz), c->d_lprobs, c->d_linact, acc}, s);
  } else if (h.segs) {
    SetsCall sc;
    sc.first = h.first, sc.segs = h.segs, sc.d_nodes = c->d_lnodes, sc.d_probs = c->d_lprobs, sc.d_inactive = c->d_linact, sc.d_acc = acc;
    rc = run_sets(c, sc, s);
  } else {
    rc = run_set(c, {h.first, h.count, c->d_lnodes, h.len, c->d_lprobs, c->d_linact, acc}, s);
  }
  if (rc) {
    hipStreamSynchronize(s);
    return rc;
  }
  if (nnz && h.probs) HIP_TRY(hipMemcpyAsync(h.probs, c->d_lprobs, sizeof(float) * nnz, hipMemcpyDeviceToHost, s));
  if (count && h.inactive) HIP_TRY(hipMemcpyAsync(h.inactive, c->d_linact, sizeof(float) * count, hipMemcpyDeviceToHost, s));
  if (nnz && h.acc) HIP_TRY(hipMemcpyAsync(h.acc, d_acc, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FDNN_OK;
}

}  // namespace fdnn
