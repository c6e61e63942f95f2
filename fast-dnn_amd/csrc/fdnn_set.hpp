// fdnn_set.hpp -- the HIP-free half of lazy output for a SHARED NODE SET (fdnn_set.hip): the guard that turns a caller's
// node into the byte offset of its weight row -- or into the offset that reads zeros --, and the tile and grid arithmetic
// of a (count rows) x (len nodes) call.  tests/host/set_check.cpp builds this header alone, under the sanitizers.
//
// A set call is LazyOutputActivations (src/cpp/dnn.cc:355-392) with ONE active list for a whole row range:
//   nodes[len] int32, strictly ascending, each in [0, output_dim); results probs [count][len] and inactive [count].
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FDNN_SET_HD __host__ __device__
#else
#define FDNN_SET_HD
#endif

namespace fdnn {
namespace set {

constexpr int kNodeTile = 64;    // NT: gathered nodes per tile (two 32-row MFMA tiles)
constexpr int kFrameTile = 32;   // FT: frames per tile
constexpr int kMaxK = 2048;      // the K the kernel stages at once: 8 waves x 256 bytes
// A buffer offset past every descriptor of the kernel: such a lane fetches nothing and its LDS bytes read as zeros.
constexpr int kOutOfRange = 0x7ffffff0;

FDNN_SET_HD inline bool node_ok(int32_t node, int rows) { return static_cast<uint32_t>(node) < static_cast<uint32_t>(rows); }

// Byte offset of weight row `node` inside the layer's [rows][ldw] image, or kOutOfRange for a node that is not a row of the
// layer (the device form does not validate its set) and for the slots past `len` of the last node tile (node = -1).
FDNN_SET_HD inline int row_offset(int32_t node, int rows, int ldw) { return node_ok(node, rows) ? node * ldw : kOutOfRange; }

// Does the MFMA kernel's shape apply to this layer?  The whole K in one pass, every row offset below the sentinel.
inline bool shape_applies(int K, int rows, int ldw, int lda) {
  return K > 0 && K <= kMaxK && K % 16 == 0 && K <= ldw && K <= lda && static_cast<long long>(rows) * ldw < kOutOfRange &&
         static_cast<long long>(kFrameTile) * lda < kOutOfRange;
}

// The grid of a call: node tiles x frame groups; a workgroup keeps its node tile's weights in registers and walks the
// frame tiles [t_begin, t_end) of its group.  As many groups as keep the launch within about one workgroup per CU.
struct Plan {
  int node_tiles, frame_tiles, groups, tiles_per_group, blocks;
};

inline Plan plan(int count, int len, int n_cu) {
  Plan p{0, 0, 0, 0, 0};
  if (count <= 0 || len <= 0) return p;
  p.node_tiles = (len + kNodeTile - 1) / kNodeTile;
  p.frame_tiles = (count + kFrameTile - 1) / kFrameTile;
  int want = (n_cu > 0 ? n_cu : 256) / p.node_tiles;
  want = want < 1 ? 1 : want > p.frame_tiles ? p.frame_tiles : want;
  p.tiles_per_group = (p.frame_tiles + want - 1) / want;
  p.groups = (p.frame_tiles + p.tiles_per_group - 1) / p.tiles_per_group;
  p.blocks = p.node_tiles * p.groups;
  return p;
}

// Workgroup `block` of the plan: entries [m0, m0 + kNodeTile) of the set, frame tiles [t_begin, t_end).  The node tiles
// of one frame group are neighbours in launch order: they read the same activation rows.
struct Tile {
  int m0, t_begin, t_end;
};

FDNN_SET_HD inline Tile block_tile(const Plan &p, int block) {
  const int mt = block % p.node_tiles, fg = block / p.node_tiles;
  const int t_begin = fg * p.tiles_per_group;
  const int t_end = t_begin + p.tiles_per_group < p.frame_tiles ? t_begin + p.tiles_per_group : p.frame_tiles;
  return Tile{mt * kNodeTile, t_begin, t_end};
}

}  // namespace set
}  // namespace fdnn
