// fdnn_half_set.hpp -- the HIP-free half of LAZY OUTPUT FOR PER-SEGMENT NODE SETS ON THE HALF NET (fdnn_half_set.hip): the
// contract, the shape rule, the LDS image of the resident weight tile, the node guard and the grid arithmetic over a
// launch table.  fdnn_half_api.cpp holds the C-ABI; DESIGN section 34.
//
// THE CONTRACT
//   tables       those of fdnn_calculate_lazy_sets (fdnn_sets.hpp): seg_rows [n_segs + 1] and set_ptr [n_segs + 1], host memory
//                in every form, and nodes.  Sets ascend strictly inside [0, O); empty segments and empty sets are allowed.
//                probs is ragged: block s is [rows_s][len_s] at sum_{t < s} rows_t len_t; inactive holds one value per row.
//                sets::check, sets::slice and sets::row_ptr are used as they stand.
//   a listed     z = RN32(s + bias), s the half net's sum under THE CONTRACT of fdnn_half.hpp: v_mfma_f32_32x32x16_f16 with
//   node         A = the W fragment and B = the X fragment, a lane's k = 16 kk + 8 (lane >> 5) + 0 .. 7, kk ascending, ONE
//                accumulator chain per output from +0, no split-K, no per-wave k halves; W pad columns are -0 and no k past
//                K_pad enters a sum.  e = exp2(RN(z RN32(log2 e))), unstabilised, as in the dense output form.
//   the rest     every unlisted node has logit 0 and contributes 1.  The total, inactive = 1 / total and p = e inactive are
//                launch_lists_finish's (fdnn_lists.hip) over the ragged row pointer, rows = O: no third order of additions.
//   so           a row's bytes are a function of the row, its set and the model alone: not of n, the chunk, the segment
//                layout, the small setting or the entry point.
//   dense bytes  the logit of (row, listed node) has the bytes of the dense kernels' tap z of that node and row: the same
//                instruction, operand roles and k order; a gathered node sits in row (position in the set) mod 32 of the
//                A fragment, not node mod 32 (held by tests/test_gpu_half_set.py).
//   a bad node   (the device form does not validate its sets) reads no weights and makes its entry, hence its segment's rows,
//                NaN and no others.
//
// THE LDS IMAGE of the workgroup's 32 gathered weight rows (K_pad <= 2048): kWBlocks = 8 blocks of 32 rows x 256 k in
// hsmall_kernel's tile image (fdnn_half_small.hip).  One direct global-to-LDS load writes a wave's 64 x 16 bytes
// contiguously: a PIECE is rows r and r + 16 of the tile (r = 0 .. 15), 256 k = 32 slots of 16 bytes each, lane l taking
// slot l & 31 of row r + 16 (l >> 5) -- each lane with its OWN row base, the gather.  Pieces are 65 slots apart (one of
// padding), so row r of a block is at slot 65 (r & 15) + 32 (r >> 4) + c, a block is 16 x 1040 = 16 640 bytes and the tile
// 133 120 of gfx950's 163 840.  A fragment read (ds_read_b128) takes the SAME c of 32 consecutive rows per half wave; the
// LDS serves it in groups of 16 consecutive lanes = 16 consecutive rows with one r >> 4, at slots 65 r' + const, r' = 0 ..
// 15: 65 = 1 mod 16, so the 16 lanes fall on 16 distinct 16-byte slots of the 64 banks x 4 bytes -- no conflict, against
// the 16-way one of rows 512 bytes apart.
#pragma once
#include "fdnn_sets.hpp"

namespace fdnn {
namespace hset {

constexpr int kNodeTile = 32;    // gathered nodes per workgroup: one A fragment's rows
constexpr int kFrameTile = 32;   // frames per tile: one B fragment's rows
constexpr int kMaxK = 2048;      // the K_pad whose 32 rows stay in LDS
constexpr int kBlockK = 256;     // k per block of the image
constexpr int kPieceStride = 1040;                    // bytes between pieces: 65 slots
constexpr int kBlockBytes = 16 * kPieceStride;        // 32 rows x 256 k and 16 slots of padding
constexpr int kWBlocks = kMaxK / kBlockK;
constexpr int kWBytes = kWBlocks * kBlockBytes;       // 133 120
constexpr int kLdsBytes = kWBytes + 4 * kNodeTile;    // ... and the tile's 32 biases (NaN for a bad node)
constexpr int kNoRead = static_cast<int>(0x80000000u);  // a byte offset past every descriptor's extent: the load writes zeros
static_assert(kLdsBytes <= 160 * 1024, "the resident tile exceeds the CU's LDS");
static_assert(kPieceStride % 16 == 0 && (kPieceStride / 16) % 16 == 1, "pieces 1 mod 16 slots apart: 16 rows, 16 distinct slots");

// 16-byte slot of (row r of the tile, slot c of its 256 k) inside a block
constexpr int w_slot(int r, int c) { return 65 * (r & 15) + 32 * (r >> 4) + c; }

// Does the resident-tile kernel serve this output layer?  Else the dense exp launch and a gather do (the same bytes).
inline bool applies(int K_pad, int rows_pad, int lda, int chunk_rows) {
  return K_pad > 0 && K_pad <= kMaxK && K_pad % 32 == 0 && lda >= K_pad && 2ll * rows_pad * K_pad < 0x7fffffffll &&
         2ll * chunk_rows * lda < 0x7fffffffll;
}

// Byte offset of weight row `node` in the layer's f16 [rows_pad][K_pad] image, or kNoRead for a node that is not a row of
// the layer and for the slots past `len` of a set's last tile (node = -1).
FDNN_SET_HD inline int row_offset(int32_t node, int rows, int K_pad) { return set::node_ok(node, rows) ? node * K_pad * 2 : kNoRead; }

// The device form's check: the tables alone (sets::check without the nodes).  0, or -(s + 1) of the first bad segment.
inline int check_tables(const int32_t *seg_rows, const int32_t *set_ptr, int n_segs, int output_dim, int rows) {
  if (n_segs <= 0) return 0;
  if (!seg_rows || !set_ptr || seg_rows[0] < 0 || set_ptr[0] != 0) return -1;
  for (int s = 0; s < n_segs; ++s)
    if (seg_rows[s + 1] < seg_rows[s] || seg_rows[s + 1] > rows || set_ptr[s + 1] < set_ptr[s] || set_ptr[s + 1] - set_ptr[s] > output_dim) return -(s + 1);
  return 0;
}

inline int node_tiles(int len) { return (len + kNodeTile - 1) / kNodeTile; }
inline int frame_tiles(int rows) { return (rows + kFrameTile - 1) / kFrameTile; }

inline int blocks_of(const sets::Seg &g, int tiles_per_group) {
  if (g.rows <= 0 || g.len <= 0) return 0;  // nothing to score: the finish pass writes such a row's 1 / output_dim
  return node_tiles(g.len) * ((frame_tiles(g.rows) + tiles_per_group - 1) / tiles_per_group);
}

// The launches of a call, laid out like sets::plan: sets::kMaxSegs segments each, in order, the table passed by value.
// ONE tiles_per_group for the call: a workgroup pays for its 32 rows once, so it takes at least four frame tiles (one per
// wave) where a segment has them, and more where a launch would otherwise have more workgroups than CUs.
inline std::vector<sets::Launch> plan(const std::vector<sets::Seg> &segs, int n_cu) {
  const int cus = n_cu > 0 ? n_cu : 256;
  int most_tiles = 1;
  for (const sets::Seg &g : segs)
    if (g.len > 0 && frame_tiles(g.rows) > most_tiles) most_tiles = frame_tiles(g.rows);
  int tpg = most_tiles < 4 ? most_tiles : 4;
  for (; tpg < most_tiles; ++tpg) {
    bool fits = true;
    for (size_t s0 = 0; s0 < segs.size() && fits; s0 += sets::kMaxSegs) {
      long long blocks = 0;
      for (size_t s = s0; s < segs.size() && s < s0 + sets::kMaxSegs; ++s) blocks += hset::blocks_of(segs[s], tpg);
      fits = blocks <= cus;
    }
    if (fits) break;
  }
  std::vector<sets::Launch> out;
  for (size_t s0 = 0; s0 < segs.size(); s0 += sets::kMaxSegs) {
    sets::Launch l{};
    l.tiles_per_group = tpg;
    for (size_t s = s0; s < segs.size() && s < s0 + sets::kMaxSegs; ++s) {
      const int i = l.n_segs++;
      l.row0[i] = segs[s].row0, l.rows[i] = segs[s].rows, l.set_off[i] = segs[s].set_off, l.len[i] = segs[s].len, l.out_off[i] = segs[s].out_off;
      l.block_off[i + 1] = l.block_off[i] + hset::blocks_of(segs[s], tpg);
    }
    for (int i = l.n_segs; i < sets::kMaxSegs; ++i) l.block_off[i + 1] = l.block_off[l.n_segs];
    out.push_back(l);
  }
  return out;
}

// Workgroup `block` of a launch: its segment (the last s with block_off[s] <= block), entries [m0, m0 + 32) of that
// segment's set and its frame tiles [t_begin, t_end), counted from the segment's own first row.  No tile crosses a segment.
FDNN_SET_HD inline sets::Tile block_tile(const sets::Launch &l, int block) {
  int lo = 0, hi = l.n_segs;  // block_off[lo] <= block < block_off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (l.block_off[mid] <= block)
      lo = mid;
    else
      hi = mid;
  }
  const int local = block - l.block_off[lo];
  const int nt = (l.len[lo] + kNodeTile - 1) / kNodeTile, ft = (l.rows[lo] + kFrameTile - 1) / kFrameTile;
  const int mt = local % nt, fg = local / nt;
  const int t_begin = fg * l.tiles_per_group;
  const int t_end = t_begin + l.tiles_per_group < ft ? t_begin + l.tiles_per_group : ft;
  return sets::Tile{lo, mt * kNodeTile, t_begin, t_end};
}

}  // namespace hset
}  // namespace fdnn

// ---------------------------------------------------------------- launch interface of fdnn_half_set.hip
struct ihipStream_t;
namespace fdnn {
namespace hset {

// The output layer on the listed nodes of one chunk's slice: e = exp(z) of (row r, entry j) of segment s to
// probs[out_off_s + r len_s + j], z to the same place of `z` unless null.
struct Params {
  const uint16_t *a;     // f16 [m][lda] the slice's last hidden rows; columns [0, K_pad) read
  const uint16_t *w;     // f16 [rows_pad][K_pad]
  const float *bias;     // [rows_pad]
  const int32_t *nodes;  // the call's whole node array (not validated: row_offset's guard)
  float *probs, *z;      // the slice's first block
  int rows, rows_pad, K_pad, lda;
};
void launch_score(const Params &p, const sets::Launch &l, ihipStream_t *s);
// The fallback (K_pad > kMaxK): e [m][rows] (and zd, the dense tap, unless null) of the chunk's dense exp launch -> the listed
// entries, NaN for a bad node.
void launch_gather(const Params &p, const float *e, const float *zd, const sets::Launch &l, ihipStream_t *s);
// set.score, set.score.tap, set.gather
constexpr int kLaunchKinds = 3;
void launch_counts(unsigned long long out[kLaunchKinds]);

}  // namespace hset
}  // namespace fdnn
