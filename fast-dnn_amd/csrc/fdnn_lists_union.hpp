// fdnn_lists_union.hpp -- the HIP-free half of lazy output by lists scored over PER-FRAME-GROUP NODE UNIONS
// (fdnn_lists_union.hip): when the path applies, how a call's rows fall into groups, what the path keeps in a context and
// where, the bound of the score grid, and a plain restatement of what the union-build kernel writes.
// tests/host/lists_union_check.cpp builds this header alone, under the sanitizers.
//
// A list call is LazyOutputActivations (src/cpp/dnn.cc:355-392) with a list per row (fdnn_lists.hpp).  Neighbouring
// frames of a decoder's beam share most of their nodes, so the union of 32 * g consecutive rows' lists is little longer than
// one row's list: the union is scored as a SET for those rows on the int8 MFMA (fdnn_set_tile.hpp), and only the entries
// the caller listed are handed back.  Group q of a call is rows [q * 32 g, (q + 1) * 32 g) counted from the call's first row;
// its entries are the flat range [row_ptr[first row], row_ptr[last row + 1]), values clamped to [0, nnz].
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "fdnn_set.hpp"

namespace fdnn {
namespace lunion {

constexpr int kMaxGroupTiles = 8;      // g: frame tiles (of set::kFrameTile rows) per group
constexpr int kDefaultGroupTiles = 1;  // what fdnn_model_set_lists_union(m, -1) selects: measured, DESIGN.md section 16
constexpr int kBitWord = 32;           // the union bitset's word
constexpr int kMaxNodes = 65536;       // output_dim the bitset is laid out for: 2048 words and their ranks in LDS, 16 KiB
constexpr int kMaxWords = kMaxNodes / kBitWord;

// The switch's value -> g, or -1 for a value the switch does not take.  0 = off.
inline int group_tiles_of(int value) { return value == -1 ? kDefaultGroupTiles : value >= 0 && value <= kMaxGroupTiles ? value : -1; }

// Does the union path serve a call on this layer?  The set tile's own rule, and an output_dim the bitset holds.
inline bool shape_applies(int K, int rows, int ldw, int lda) { return rows > 0 && rows <= kMaxNodes && set::shape_applies(K, rows, ldw, lda); }

FDNN_SET_HD inline int group_rows(int group_tiles) { return set::kFrameTile * group_tiles; }
inline int groups(int count, int group_tiles) { return count <= 0 ? 0 : (count + group_rows(group_tiles) - 1) / group_rows(group_tiles); }

// The work list's capacity, and the most workgroups a score launch can use: summed over the groups,
// ceil(u_len / 64) <= nnz / 64 + groups, because a group's union is no longer than its entry range and the ranges are disjoint.
inline long long grid_bound(long long nnz, int n_groups) { return nnz / set::kNodeTile + n_groups; }

FDNN_SET_HD inline int clamp_ptr(int32_t v, int nnz) { return v < 0 ? 0 : v > nnz ? nnz : v; }

// A group's entry range from the caller's row_ptr: values clamped to [0, nnz], an end below its begin is the begin.
struct Range {
  int b, e;
};
FDNN_SET_HD inline Range group_range(const int32_t *row_ptr, int count, int nnz, int group_tiles, int group) {
  const int r0 = group * group_rows(group_tiles);
  const int r1 = r0 + group_rows(group_tiles) < count ? r0 + group_rows(group_tiles) : count;
  const int b = clamp_ptr(row_ptr[r0], nnz), e = clamp_ptr(row_ptr[r1], nnz);
  return Range{b, e < b ? b : e};
}

// What the path keeps in a context: one int32 buffer, offsets in words.  O(nnz + count).
//   u_nodes [nnz]         group q's union, ascending, at u_nodes + (its range's begin)
//   pos     [nnz]         every entry's rank in its group's union, -1 for a node outside [0, output_dim)
//   u_len   [groups]      the unions' lengths
//   work    [2 * bound]   (group, 64-node chunk) pairs in the order the groups appended them
//   counter [1]           work items appended (zero when the build kernel starts)
struct Layout {
  size_t u_nodes, pos, u_len, work, counter, words;
  long long bound;
  int n_groups;
};
inline Layout layout(long long nnz, int count, int group_tiles) {
  Layout l{};
  const size_t n = size_t(nnz < 0 ? 0 : nnz);
  l.n_groups = groups(count, group_tiles);
  l.bound = grid_bound(static_cast<long long>(n), l.n_groups);
  l.u_nodes = 0;
  l.pos = l.u_nodes + n;
  l.u_len = l.pos + n;
  l.work = l.u_len + size_t(l.n_groups);
  l.counter = l.work + 2 * size_t(l.bound);
  l.words = l.counter + 1;
  return l;
}

// What the union-build kernel writes, restated: u_len [groups], u_nodes [nnz] (group q's union at its range's begin; words
// no union covers are left alone), pos [nnz] (entries outside every group's range are left alone).  Returns the number of
// work items (the sum of ceil(u_len / 64)).  Nothing outside the sizes above is touched, whatever row_ptr and nodes hold.
inline long long union_ref(const int32_t *row_ptr, const int32_t *nodes, int count, int nnz, int output_dim, int group_tiles, int32_t *u_len,
                           int32_t *u_nodes, int32_t *pos) {
  long long items = 0;
  const int n_groups = groups(count, group_tiles);
  const size_t words = size_t(output_dim > 0 ? (output_dim + kBitWord - 1) / kBitWord : 0);
  std::vector<uint32_t> bits(words);
  std::vector<int32_t> rank(words);
  for (int q = 0; q < n_groups; ++q) {
    const Range r = group_range(row_ptr, count, nnz, group_tiles, q);
    for (size_t w = 0; w < words; ++w) bits[w] = 0;
    for (int i = r.b; i < r.e; ++i)
      if (set::node_ok(nodes[i], output_dim)) bits[size_t(nodes[i]) / kBitWord] |= 1u << (nodes[i] % kBitWord);
    int32_t len = 0;
    for (size_t w = 0; w < words; ++w) {
      rank[w] = len;
      for (int b = 0; b < kBitWord; ++b)
        if (bits[w] >> b & 1u) u_nodes[size_t(r.b) + size_t(len++)] = int32_t(w * kBitWord) + b;
    }
    for (int i = r.b; i < r.e; ++i) {
      if (!set::node_ok(nodes[i], output_dim)) {
        pos[i] = -1;
        continue;
      }
      const size_t w = size_t(nodes[i]) / kBitWord;
      const uint32_t below = bits[w] & ((1u << (nodes[i] % kBitWord)) - 1u);
      int32_t c = 0;
      for (int b = 0; b < kBitWord; ++b) c += int32_t(below >> b & 1u);
      pos[i] = rank[w] + c;
    }
    u_len[q] = len;
    items += (len + set::kNodeTile - 1) / set::kNodeTile;
  }
  return items;
}

}  // namespace lunion
}  // namespace fdnn
