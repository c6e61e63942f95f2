// fdnn_lists.hpp -- the host half of lazy output by active-node LISTS (fdnn_lists.hip): the validator of a caller's lists
// and the per-node index of the output layer's saturating pairs.  No HIP here: tests/host/lists_check.cpp builds this
// header alone, under the sanitizers.
//
// An active list replaces a mask (LazyOutputActivations, src/cpp/dnn.cc:355-392: the nodes a decoder asks for).  For
// `count` rows:   row_ptr[count + 1]  int32, row_ptr[0] == 0, non-decreasing, row_ptr[count] == nnz
//                 nodes[nnz]          int32, strictly ascending inside a row, each in [0, output_dim)
// -- exactly a mask per row, in CSR form.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "fdnn_model.hpp"  // FixEntry

namespace fdnn {
namespace lists {

// 0 = the lists are well formed, else -(row + 1) of the first row that is not: its range runs backwards or past what came
// before (row 0 also answers for row_ptr[0] != 0), or one of its nodes is outside [0, output_dim) or not above the node
// before it (or it has nodes and `nodes` is null).  Nothing past a row's own range is read: nodes needs row_ptr[count] entries only if every row before holds.
inline int check(const int32_t *row_ptr, const int32_t *nodes, int count, int output_dim) {
  if (count <= 0) return 0;
  if (row_ptr[0] != 0) return -1;
  for (int r = 0; r < count; ++r) {
    const int32_t b = row_ptr[r], e = row_ptr[r + 1];
    if (e < b || (e > b && !nodes)) return -(r + 1);
    int32_t prev = -1;
    for (int32_t i = b; i < e; ++i) {
      const int32_t v = nodes[i];
      if (v < 0 || v >= output_dim || v <= prev) return -(r + 1);
      prev = v;
    }
  }
  return 0;
}

// One saturating pair of a node as the score kernel reads it: k (the even column) | w0 << 16 | w1 << 24.
inline uint32_t pack_pair(const FixEntry &e) { return uint32_t(e.k) | uint32_t(uint8_t(e.w0)) << 16 | uint32_t(uint8_t(e.w1)) << 24; }

// The blob keeps a layer's FixEntry list per 64-node group, sorted by k inside a group (the GEMMs consume it as their
// k-loop brings the columns through LDS).  A list call scores single nodes, so it wants a node's pairs side by side:
// off[rows + 1] entry range of every node, pairs[n_fix] packed as above, a node's pairs in k order.  grp has
// rows_pad / 64 + 1 entries.  The blob itself is not touched.
inline void build_node_fix_index(const FixEntry *ent, const int32_t *grp, int rows, int rows_pad, std::vector<int32_t> *off,
                                 std::vector<uint32_t> *pairs) {
  const int groups = rows_pad / 64;
  const int32_t n_fix = grp[groups];
  off->assign(size_t(rows) + 1, 0);
  pairs->assign(size_t(n_fix), 0u);
  for (int32_t e = 0; e < n_fix; ++e)
    if (ent[e].node >= 0 && ent[e].node < rows) ++(*off)[size_t(ent[e].node) + 1];
  for (int r = 0; r < rows; ++r) (*off)[size_t(r) + 1] += (*off)[size_t(r)];
  std::vector<int32_t> fill(off->begin(), off->end() - 1);
  for (int32_t e = 0; e < n_fix; ++e)  // in list order: inside a group ascending k, so ascending k per node
    if (ent[e].node >= 0 && ent[e].node < rows) (*pairs)[size_t(fill[size_t(ent[e].node)]++)] = pack_pair(ent[e]);
  pairs->resize(size_t((*off)[size_t(rows)]));
}

// The slice [r0, r0 + cnt) of a call's lists as lists of its own: row_ptr rebased to 0 (the nodes are the caller's
// nodes + row_ptr[r0], unchanged).
inline void rebase_rows(const int32_t *row_ptr, int r0, int cnt, std::vector<int32_t> *out) {
  out->resize(size_t(cnt) + 1);
  for (int i = 0; i <= cnt; ++i) (*out)[size_t(i)] = row_ptr[r0 + i] - row_ptr[r0];
}

}  // namespace lists
}  // namespace fdnn
