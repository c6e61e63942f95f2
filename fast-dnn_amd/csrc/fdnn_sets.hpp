// fdnn_sets.hpp -- the HIP-free half of lazy output for PER-SEGMENT NODE SETS (fdnn_sets.hip): the validator of a caller's
// segment tables, the by-value launch table that carries up to kMaxSegs segments into one launch of the set kernel's tile,
// the grid arithmetic over it, and the slices of a call that the chunked one-call form and the scoring loop score.
// tests/host/sets_check.cpp builds this header alone, under the sanitizers.  The node guard, the tile sizes and the shape
// rule are fdnn_set.hpp's, unchanged.
//
// A sets call is LazyOutputActivations (src/cpp/dnn.cc:355-392) with one active list per SEGMENT of a row range:
//   seg_rows [n_segs + 1] int32 (host)  non-decreasing; segment s = rows [seg_rows[s], seg_rows[s + 1]) of the context
//   set_ptr  [n_segs + 1] int32 (host)  set_ptr[0] == 0, non-decreasing; segment s's set = nodes[set_ptr[s] .. set_ptr[s + 1])
//   nodes    [set_ptr[n_segs]] int32    strictly ascending inside a segment's set, each in [0, output_dim)
//   probs    ragged: segment s's block starts at sum_{t < s} rows_t * len_t and is [rows_s][len_s] row-major
//   inactive [seg_rows[n_segs] - seg_rows[0]], one value per row in row order
// -- the list contract's CSR (fdnn_lists.hpp) with row_ptr[r] = block start + r_local * len_s.
#pragma once
#include <cstdint>
#include <vector>

#include "fdnn_set.hpp"

namespace fdnn {
namespace sets {

constexpr int kMaxSegs = 64;  // segments per launch: longer tables go as several launches

struct Tables {
  const int32_t *seg_rows, *set_ptr;
  int n_segs;
};

// 0 = the tables are well formed, else -(s + 1) of the first segment that is not: its rows run backwards or past the
// context, its set's range runs backwards, or one of its nodes is outside [0, output_dim) or not above the node before it
// (or it has nodes and `nodes` is null).  Malformed tables as a whole (a null table, seg_rows[0] < 0, set_ptr[0] != 0)
// answer as segment 0.  Nothing past a segment's own range is read.
inline int check(const int32_t *seg_rows, const int32_t *set_ptr, const int32_t *nodes, int n_segs, int output_dim, int ctx_rows) {
  if (n_segs <= 0) return 0;
  if (!seg_rows || !set_ptr || seg_rows[0] < 0 || set_ptr[0] != 0) return -1;
  for (int s = 0; s < n_segs; ++s) {
    if (seg_rows[s + 1] < seg_rows[s] || seg_rows[s + 1] > ctx_rows) return -(s + 1);
    const int32_t b = set_ptr[s], e = set_ptr[s + 1];
    if (e < b || (e > b && !nodes)) return -(s + 1);
    int32_t prev = -1;
    for (int32_t i = b; i < e; ++i) {
      const int32_t v = nodes[i];
      if (v < 0 || v >= output_dim || v <= prev) return -(s + 1);
      prev = v;
    }
  }
  return 0;
}

// sum_s rows_s * len_s of checked tables: the floats of probs (a call's must fit an int32)
inline long long total(const Tables &t) {
  long long nnz = 0;
  for (int s = 0; s < t.n_segs; ++s)
    nnz += static_cast<long long>(t.seg_rows[s + 1] - t.seg_rows[s]) * (t.set_ptr[s + 1] - t.set_ptr[s]);
  return nnz;
}

// One segment of a call or of a slice of it: rows [row0, row0 + rows) counted from the slice's first row, its set
// nodes[set_off .. set_off + len), its block at probs + out_off of the SLICE's results -- and at src_off of the caller's.
struct Seg {
  int row0, rows, set_off, len, out_off, src_off;
};

// The segments of checked tables cut to context rows [row_a, row_b): rows and out_off rebased to the slice, a segment cut
// in two keeps its set, segments without a row in the slice are left out.  A slice's blocks are one contiguous range of the
// caller's probs, beginning at its first segment's src_off.
inline std::vector<Seg> slice(const Tables &t, int row_a, int row_b) {
  std::vector<Seg> out;
  long long block = 0;
  int out_off = 0;
  for (int s = 0; s < t.n_segs; ++s) {
    const int b = t.seg_rows[s], e = t.seg_rows[s + 1], len = t.set_ptr[s + 1] - t.set_ptr[s];
    const int a = b > row_a ? b : row_a, z = e < row_b ? e : row_b;
    if (a < z) {
      out.push_back(Seg{a - row_a, z - a, t.set_ptr[s], len, out_off, static_cast<int>(block + static_cast<long long>(a - b) * len)});
      out_off += (z - a) * len;
    }
    block += static_cast<long long>(e - b) * len;
  }
  return out;
}

// The list contract's row pointer of a call or slice: [rows + 1], row r of segment s at out_off_s + r * len_s.
inline std::vector<int32_t> row_ptr(const std::vector<Seg> &segs) {
  std::vector<int32_t> out;
  int32_t end = 0;
  for (const Seg &g : segs) {
    for (int r = 0; r < g.rows; ++r) out.push_back(g.out_off + r * g.len);
    end = g.out_off + g.rows * g.len;
  }
  out.push_back(end);
  return out;
}

// ... and where each row's set begins in `nodes`: [rows] (the fallback copies a row's list from there)
inline std::vector<int32_t> row_set(const std::vector<Seg> &segs) {
  std::vector<int32_t> out;
  for (const Seg &g : segs) out.insert(out.end(), static_cast<size_t>(g.rows), g.set_off);
  return out;
}

// One launch's segments, a kernel argument passed by value (1.5 KB): no table in device memory whose lifetime an enqueued
// call would have to manage.  Workgroups [block_off[s], block_off[s + 1]) belong to segment s: its node tiles x its frame
// groups of tiles_per_group frame tiles, frame tiles counted from the segment's own first row.
struct Launch {
  int n_segs, tiles_per_group;
  int row0[kMaxSegs], rows[kMaxSegs], set_off[kMaxSegs], len[kMaxSegs], out_off[kMaxSegs];
  int block_off[kMaxSegs + 1];
};

inline int node_tiles(int len) { return (len + set::kNodeTile - 1) / set::kNodeTile; }
inline int frame_tiles(int rows) { return (rows + set::kFrameTile - 1) / set::kFrameTile; }

inline int blocks_of(const Seg &g, int tiles_per_group) {
  if (g.rows <= 0 || g.len <= 0) return 0;  // nothing to score: the finish pass writes such a row's 1 / output_dim
  return node_tiles(g.len) * ((frame_tiles(g.rows) + tiles_per_group - 1) / tiles_per_group);
}

// The launches of a call: kMaxSegs segments each, in order.  ONE tiles_per_group for the whole call: the smallest with
// which no launch has more workgroups than CUs -- or every workgroup already walks all frame tiles of its segment.
inline std::vector<Launch> plan(const std::vector<Seg> &segs, int n_cu) {
  const int cus = n_cu > 0 ? n_cu : 256;
  int most_tiles = 1;
  for (const Seg &g : segs)
    if (g.len > 0) most_tiles = frame_tiles(g.rows) > most_tiles ? frame_tiles(g.rows) : most_tiles;
  int tpg = 1;
  for (; tpg < most_tiles; ++tpg) {
    bool fits = true;
    for (size_t s0 = 0; s0 < segs.size() && fits; s0 += kMaxSegs) {
      long long blocks = 0;
      for (size_t s = s0; s < segs.size() && s < s0 + kMaxSegs; ++s) blocks += blocks_of(segs[s], tpg);
      fits = blocks <= cus;
    }
    if (fits) break;
  }
  std::vector<Launch> out;
  for (size_t s0 = 0; s0 < segs.size(); s0 += kMaxSegs) {
    Launch l{};
    l.tiles_per_group = tpg;
    for (size_t s = s0; s < segs.size() && s < s0 + kMaxSegs; ++s) {
      const int i = l.n_segs++;
      l.row0[i] = segs[s].row0, l.rows[i] = segs[s].rows, l.set_off[i] = segs[s].set_off, l.len[i] = segs[s].len, l.out_off[i] = segs[s].out_off;
      l.block_off[i + 1] = l.block_off[i] + blocks_of(segs[s], tpg);
    }
    for (int i = l.n_segs; i < kMaxSegs; ++i) l.block_off[i + 1] = l.block_off[l.n_segs];
    out.push_back(l);
  }
  return out;
}

inline int blocks(const Launch &l) { return l.block_off[l.n_segs]; }

// Workgroup `block` of a launch: the segment it belongs to (the last s with block_off[s] <= block: segments without
// workgroups are stepped over), entries [m0, m0 + kNodeTile) of that segment's set and its frame tiles [t_begin, t_end).
// No tile crosses a segment.  The node tiles of one frame group are neighbours in launch order.
struct Tile {
  int seg, m0, t_begin, t_end;
};

FDNN_SET_HD inline Tile block_tile(const Launch &l, int block) {
  int lo = 0, hi = l.n_segs;  // block_off[lo] <= block < block_off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (l.block_off[mid] <= block)
      lo = mid;
    else
      hi = mid;
  }
  const int local = block - l.block_off[lo];
  const int nt = (l.len[lo] + set::kNodeTile - 1) / set::kNodeTile, ft = (l.rows[lo] + set::kFrameTile - 1) / set::kFrameTile;
  const int mt = local % nt, fg = local / nt;
  const int t_begin = fg * l.tiles_per_group;
  const int t_end = t_begin + l.tiles_per_group < ft ? t_begin + l.tiles_per_group : ft;
  return Tile{lo, mt * set::kNodeTile, t_begin, t_end};
}

}  // namespace sets
}  // namespace fdnn
