// set_check.cpp -- the host half of lazy output for a shared node set (fdnn_set.hpp), checked without a GPU: the guard that
// turns a caller's node into a weight-row offset or the offset that reads zeros, and the tile plan of a (count, len) call --
// every (row, entry) is covered by exactly one workgroup's tiles.  Built with -fsanitize=address,undefined and run as a
// child process by tests/test_lazy_set_host.py; exit status 0 = all cases hold.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fdnn_set.hpp"

using namespace fdnn;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

namespace {

// rows x ldw is the layer's image: an offset is valid when the whole row [off, off + ldw) lies inside it
void guard() {
  const struct {
    int rows, ldw;
  } layers[] = {{1000, 320}, {8000, 2112}, {251, 320}, {1, 144}, {100, 144}};
  for (const auto &l : layers) {
    const int O = l.rows;
    CHECK(set::shape_applies(l.ldw - 64, O, l.ldw, l.ldw));
    const long long image = static_cast<long long>(O) * l.ldw;
    CHECK(image < set::kOutOfRange);  // the sentinel is past the descriptor: such a lane fetches nothing
    const int32_t bad[] = {-1, O, O + 1, INT32_MAX, INT32_MIN, INT32_MIN + 1, -O, 1 << 30};
    for (int32_t v : bad) {
      CHECK(!set::node_ok(v, O));
      CHECK(set::row_offset(v, O, l.ldw) == set::kOutOfRange);
    }
    const int32_t good[] = {0, O - 1, O / 2};
    for (int32_t v : good) {
      CHECK(set::node_ok(v, O));
      const int off = set::row_offset(v, O, l.ldw);
      CHECK(off == v * l.ldw && off >= 0 && static_cast<long long>(off) + l.ldw <= image);
    }
    for (int32_t v = -3; v < O + 3; ++v) {  // every node around and inside the layer
      const int off = set::row_offset(v, O, l.ldw);
      CHECK((v >= 0 && v < O) ? (off == v * l.ldw) : (off == set::kOutOfRange));
    }
  }
  // layers the kernel must not be given: K past what it stages, an image that reaches the sentinel
  CHECK(!set::shape_applies(set::kMaxK + 128, 1000, set::kMaxK + 192, set::kMaxK + 192));
  CHECK(!set::shape_applies(2048, 1100000, 2112, 2112));
  CHECK(!set::shape_applies(0, 1000, 320, 320));
  CHECK(set::shape_applies(2048, 8000, 2112, 2112));
}

// every (row, entry) of the call in exactly one (workgroup, frame tile), no tile outside the plan's ranges
void cover(int count, int len, int n_cu) {
  const set::Plan p = set::plan(count, len, n_cu);
  if (count <= 0 || len <= 0) {
    CHECK(p.blocks == 0);
    return;
  }
  CHECK(p.node_tiles == (len + set::kNodeTile - 1) / set::kNodeTile && p.frame_tiles == (count + set::kFrameTile - 1) / set::kFrameTile);
  CHECK(p.groups >= 1 && p.tiles_per_group >= 1 && p.blocks == p.node_tiles * p.groups);
  CHECK(static_cast<long long>(p.groups) * p.tiles_per_group >= p.frame_tiles);
  CHECK(static_cast<long long>(p.groups - 1) * p.tiles_per_group < p.frame_tiles);  // no workgroup without a tile
  std::vector<unsigned char> seen(static_cast<size_t>(count) * len, 0);
  for (int b = 0; b < p.blocks; ++b) {
    const set::Tile t = set::block_tile(p, b);
    CHECK(t.m0 >= 0 && t.m0 < len && t.m0 % set::kNodeTile == 0);
    CHECK(0 <= t.t_begin && t.t_begin < t.t_end && t.t_end <= p.frame_tiles);
    for (int ft = t.t_begin; ft < t.t_end; ++ft)
      for (int f = 0; f < set::kFrameTile; ++f) {
        const int row = ft * set::kFrameTile + f;
        if (row >= count) continue;  // rows past the call: read as zeros, nothing stored
        for (int j = t.m0; j < t.m0 + set::kNodeTile && j < len; ++j) {
          unsigned char &s = seen[static_cast<size_t>(row) * len + j];
          CHECK(s == 0);
          s = 1;
        }
      }
  }
  for (unsigned char s : seen) CHECK(s == 1);
}

}  // namespace

int main() {
  guard();
  const int cus[] = {1, 8, 256};
  for (int n_cu : cus)
    for (int count = 0; count <= 70; ++count)
      for (int len = 0; len <= 70; ++len) cover(count, len, n_cu);
  cover(8000, 8000, 256);
  cover(8000, 1, 256);
  cover(1, 8000, 256);
  cover(10000, 80, 0);  // an unknown CU count plans for 256
  std::printf("set ok\n");
  return 0;
}
