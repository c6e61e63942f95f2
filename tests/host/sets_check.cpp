// sets_check.cpp -- the host half of lazy output for per-segment node sets (fdnn_sets.hpp) and the scoring loop's plan for
// set submissions (fdnn_server_plan.hpp: Want::set), checked without a GPU: the validator on every class of malformed tables; the
// launches of a call -- every (row, entry) of every segment covered by exactly one workgroup's tiles, no tile across a
// segment, at most 64 segments per launch; the slices of a call reassembling to the unsliced layout; the row pointer; and
// that set requests share batches only with set requests, a split request continuing at taken * len.  Built with
// -fsanitize=address,undefined and run as a child process by tests/test_lazy_sets_host.py; exit status 0 = all cases hold.
// `sets_check rowptr <seg_rows..> / <set_ptr..>` prints sets::row_ptr of the tables (the test compares formats.sets_to_lists).
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <random>
#include <vector>

#include "fdnn_server_plan.hpp"
#include "fdnn_sets.hpp"

using namespace fdnn;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

namespace {

using V = std::vector<int32_t>;

int chk(const V &seg_rows, const V &set_ptr, const V &nodes, int O, int ctx_rows) {
  return sets::check(seg_rows.data(), set_ptr.data(), nodes.empty() ? nullptr : nodes.data(), int(seg_rows.size()) - 1, O, ctx_rows);
}

void validator() {
  const int O = 1000;
  // what the contract allows: an empty segment, a zero-length set, node 0 and node O - 1, rows up to the context's last
  CHECK(chk({0, 1, 32, 32, 65, 100}, {0, 2, 2, 3, 5, 6}, {0, 999, 7, 1, 2, 999}, O, 100) == 0);
  CHECK(chk({5, 5}, {0, 0}, {}, O, 100) == 0);
  CHECK(sets::check(nullptr, nullptr, nullptr, 0, O, 100) == 0);  // n_segs == 0: a no-op
  // malformed tables as a whole answer as segment 0
  CHECK(sets::check(nullptr, nullptr, nullptr, 2, O, 100) == -1);
  CHECK(chk({-1, 3}, {0, 1}, {4}, O, 100) == -1);        // seg_rows[0] < 0
  CHECK(chk({0, 3, 6}, {1, 2, 3}, {4, 5, 6}, O, 100) == -1);  // set_ptr[0] != 0
  // per segment: rows backwards, rows past the context, a set's range backwards
  CHECK(chk({0, 10, 5}, {0, 1, 2}, {4, 5}, O, 100) == -2);
  CHECK(chk({0, 10, 101}, {0, 1, 2}, {4, 5}, O, 100) == -2);
  CHECK(chk({0, 10, 20, 30}, {0, 2, 1, 3}, {4, 5, 6}, O, 100) == -2);
  // per segment: unsorted, a duplicate, negative, == O, nodes without a node array
  CHECK(chk({0, 10, 20}, {0, 2, 5}, {1, 2, 3, 2, 7}, O, 100) == -2);
  CHECK(chk({0, 10, 20}, {0, 2, 5}, {1, 2, 4, 4, 7}, O, 100) == -2);
  CHECK(chk({0, 10, 20}, {0, 2, 4}, {-1, 5, 1, 2}, O, 100) == -1);
  CHECK(chk({0, 10, 20, 30}, {0, 1, 2, 4}, {1, 2, 5, O}, O, 100) == -3);
  const V sr{0, 10}, sp{0, 2};
  CHECK(sets::check(sr.data(), sp.data(), nullptr, 1, O, 100) == -1);
  // the next segment's set may begin below the last node of the one before: ascending inside a set only
  CHECK(chk({0, 10, 20}, {0, 2, 4}, {5, 9, 1, 2}, O, 100) == 0);
  // nothing past the first malformed segment is read (the sanitizers watch): nodes is as long as segment 0 needs
  CHECK(chk({0, 10, 20}, {0, 2, 900}, {9, 5}, O, 100) == -1);
}

std::vector<sets::Seg> whole(const V &seg_rows, const V &set_ptr) {
  const sets::Tables t{seg_rows.data(), set_ptr.data(), int(seg_rows.size()) - 1};
  return sets::slice(t, seg_rows.front(), seg_rows.back());
}

// every (row, entry) of every segment in exactly one (workgroup, frame tile); no tile outside its segment
void cover(const V &rows, const V &lens, int n_cu) {
  V seg_rows{0}, set_ptr{0};
  for (size_t s = 0; s < rows.size(); ++s) seg_rows.push_back(seg_rows.back() + rows[s]), set_ptr.push_back(set_ptr.back() + lens[s]);
  const std::vector<sets::Seg> segs = whole(seg_rows, set_ptr);
  long long nnz = 0;
  size_t live = 0;
  for (size_t s = 0; s < rows.size(); ++s) nnz += static_cast<long long>(rows[s]) * lens[s], live += rows[s] > 0;
  CHECK(segs.size() == live);  // segments without rows are left out
  std::vector<unsigned char> seen(static_cast<size_t>(nnz), 0);
  const std::vector<sets::Launch> launches = sets::plan(segs, n_cu);
  CHECK(launches.size() == (segs.size() + sets::kMaxSegs - 1) / sets::kMaxSegs);
  size_t s0 = 0;
  int tpg = 0;
  for (const sets::Launch &l : launches) {
    CHECK(l.n_segs >= 1 && l.n_segs <= sets::kMaxSegs && l.tiles_per_group >= 1);
    CHECK(tpg == 0 || tpg == l.tiles_per_group);  // one tiles_per_group for the whole call
    tpg = l.tiles_per_group;
    CHECK(l.block_off[0] == 0);
    for (int i = 0; i < l.n_segs; ++i) {
      const sets::Seg &g = segs[s0 + size_t(i)];
      CHECK(l.row0[i] == g.row0 && l.rows[i] == g.rows && l.set_off[i] == g.set_off && l.len[i] == g.len && l.out_off[i] == g.out_off);
      CHECK(l.block_off[i + 1] >= l.block_off[i]);
      if (g.len == 0) CHECK(l.block_off[i + 1] == l.block_off[i]);  // nothing to score: no workgroups
    }
    for (int b = 0; b < sets::blocks(l); ++b) {
      const sets::Tile t = sets::block_tile(l, b);
      CHECK(t.seg >= 0 && t.seg < l.n_segs && l.block_off[t.seg] <= b && b < l.block_off[t.seg + 1]);
      const int rws = l.rows[t.seg], len = l.len[t.seg];
      CHECK(rws > 0 && len > 0);
      CHECK(t.m0 >= 0 && t.m0 < len && t.m0 % set::kNodeTile == 0);
      CHECK(0 <= t.t_begin && t.t_begin < t.t_end && t.t_end <= sets::frame_tiles(rws));  // no workgroup without a tile
      for (int ft = t.t_begin; ft < t.t_end; ++ft)
        for (int f = 0; f < set::kFrameTile; ++f) {
          const int r = ft * set::kFrameTile + f;  // counted from the segment's own first row
          if (r >= rws) continue;                  // rows past the SEGMENT: read as zeros, nothing stored
          for (int j = t.m0; j < t.m0 + set::kNodeTile && j < len; ++j) {
            unsigned char &sn = seen[static_cast<size_t>(l.out_off[t.seg]) + static_cast<size_t>(r) * len + j];
            CHECK(sn == 0);
            sn = 1;
          }
        }
    }
    s0 += size_t(l.n_segs);
  }
  CHECK(s0 == segs.size());
  for (unsigned char sn : seen) CHECK(sn == 1);
  // about one workgroup per CU: a launch has more workgroups than CUs only where every workgroup already walks all frame
  // tiles of its segment (one workgroup per node tile is the least a segment can have)
  const int cus = n_cu > 0 ? n_cu : 256;
  int most_tiles = 1;
  for (const sets::Seg &g : segs)
    if (g.len > 0 && sets::frame_tiles(g.rows) > most_tiles) most_tiles = sets::frame_tiles(g.rows);
  for (const sets::Launch &l : launches) CHECK(sets::blocks(l) <= cus || l.tiles_per_group >= most_tiles);
}

void covers() {
  std::mt19937 rng(7);
  const int cus[] = {1, 8, 256};
  for (int n_cu : cus) {
    for (int n_segs : {1, 2, 3, 5, 63, 64, 65, 128, 129, 130}) {
      for (int rep = 0; rep < (n_segs <= 5 ? 40 : 3); ++rep) {
        V rows, lens;
        for (int s = 0; s < n_segs; ++s) {
          rows.push_back(rng() % 8 == 0 ? 0 : int(rng() % 71));
          lens.push_back(rng() % 8 == 0 ? 0 : int(rng() % 71));
        }
        cover(rows, lens, n_cu);
      }
    }
    for (int r = 0; r <= 70; ++r)  // every row count and length once against a fixed neighbour
      for (int len = 0; len <= 70; len += (r % 7 == 0 ? 1 : 9)) cover({r, 33, 1}, {len, 65, 0}, n_cu);
  }
  cover({8000, 1, 100}, {80, 8000, 8000}, 256);
  cover({1, 8000}, {8000, 1}, 0);  // an unknown CU count plans for 256
  // the issue's composition: boundaries at rows 1, 32 and 65
  cover({1, 31, 0, 33, 35}, {65, 0, 1, 129, 64}, 256);
}

// the slices of a call at every cut: rows, blocks and out_off reassemble to the unsliced layout
void slices() {
  const V seg_rows{3, 4, 35, 35, 68, 103}, set_ptr{0, 65, 65, 66, 195, 259};
  const sets::Tables t{seg_rows.data(), set_ptr.data(), 5};
  const std::vector<sets::Seg> all = whole(seg_rows, set_ptr);
  const V want_rp = sets::row_ptr(all);
  CHECK(int(want_rp.size()) == 101 && want_rp.back() == sets::total(t));
  for (int a = 3; a <= 103; ++a)
    for (int b = a; b <= 103; ++b) {
      const std::vector<sets::Seg> sl = sets::slice(t, a, b);
      if (a == b) {
        CHECK(sl.empty());
        continue;
      }
      int row = 0, out = 0;
      for (const sets::Seg &g : sl) {
        CHECK(g.rows > 0 && g.row0 == row && g.out_off == out);  // rebased to the slice, consecutive
        CHECK(g.src_off == sl[0].src_off + g.out_off);           // the slice's blocks are one contiguous range of the caller's probs
        row += g.rows, out += g.rows * g.len;
      }
      CHECK(row == b - a);
      const V rp = sets::row_ptr(sl);
      const V rs = sets::row_set(sl);
      CHECK(int(rp.size()) == b - a + 1 && int(rs.size()) == b - a);
      for (int r = 0; r < b - a; ++r) {
        CHECK(rp[size_t(r)] + sl[0].src_off == want_rp[size_t(a - 3 + r)]);  // where the unsliced call puts this row
        int s = 0;
        while (!(seg_rows[size_t(s)] <= a + r && a + r < seg_rows[size_t(s) + 1])) ++s;
        CHECK(rs[size_t(r)] == set_ptr[size_t(s)]);  // a segment cut in two keeps its set
        CHECK(rp[size_t(r) + 1] - rp[size_t(r)] == set_ptr[size_t(s) + 1] - set_ptr[size_t(s)]);
      }
    }
  // two slices side by side cover the call
  for (int cut = 3; cut <= 103; ++cut) {
    const std::vector<sets::Seg> lo = sets::slice(t, 3, cut), hi = sets::slice(t, cut, 103);
    long long n = 0;
    for (const sets::Seg &g : lo) n += static_cast<long long>(g.rows) * g.len;
    if (!hi.empty()) CHECK(hi[0].src_off == n);
    for (const sets::Seg &g : hi) n += static_cast<long long>(g.rows) * g.len;
    CHECK(n == sets::total(t));
  }
}

// the scoring loop's plan: kinds do not mix, a split request's second piece continues at taken * len
void server_plan() {
  using namespace fdnn::plan;
  const size_t O = 1000;
  float x[4], out[4], probs[4], inact[4];
  uint64_t bits[16] = {0};
  const SetRef a = std::make_shared<const std::vector<int32_t>>(std::vector<int32_t>{1, 5, 9});
  const SetRef b = std::make_shared<const std::vector<int32_t>>(std::vector<int32_t>{});
  auto set_req = [&](uint64_t ticket, int n, const SetRef &set) {
    Request r(Frames::rows(x), Want::set_to(set, probs, inact), n);
    r.ticket = ticket;
    return r;
  };
  Request dense(Frames::rows(x), Want::rows_to(out), 10);
  dense.ticket = 9;
  Request bit(Frames::rows(x), Want::rows_behind_bits_to(bits, 0, out), 10);
  bit.ticket = 10;
  CHECK(set_req(1, 5, a).want.kind == Want::set && set_req(1, 5, b).want.kind == Want::set && dense.want.kind == Want::rows && bit.want.kind == Want::rows_behind_bits);
  std::deque<Request> q{set_req(1, 40, a), set_req(2, 100, b), set_req(3, 100, a), dense, set_req(4, 7, a), bit, set_req(5, 3, a)};
  BatchPlan p = plan_batch(q, 96, O);  // 40 of a, 56 of b
  CHECK(p.kind == Want::set && p.rows == 96 && p.pieces.size() == 2 && p.nnz == 40 * 3 && p.set_nodes == 3 && p.stride == 0);
  CHECK(p.pieces[0].want.nodes == a && p.pieces[0].want.probs == probs && p.pieces[0].want.inactive == inact && p.pieces[0].block_off == 0 && p.pieces[0].last);
  CHECK(p.pieces[0].want.out == nullptr);
  CHECK(p.pieces[1].want.nodes == b && p.pieces[1].row0 == 40 && p.pieces[1].rows == 56 && !p.pieces[1].last && p.pieces[1].block_off == 120);
  p = plan_batch(q, 96, O);  // the rest of b (44), 52 of ticket 3
  CHECK(p.kind == Want::set && p.rows == 96 && p.pieces.size() == 2);
  CHECK(p.pieces[0].ticket == 2 && p.pieces[0].want.inactive == inact + 56 && p.pieces[0].last && p.pieces[0].set_off == 0 && p.pieces[0].block_off == 0);
  CHECK(p.pieces[1].ticket == 3 && p.pieces[1].rows == 52 && p.pieces[1].want.probs == probs && p.pieces[1].set_off == 0 && p.nnz == 52 * 3);
  p = plan_batch(q, 96, O);  // the rest of 3 continues at taken * len; the dense request behind it does not join
  CHECK(p.kind == Want::set && p.pieces.size() == 1 && p.rows == 48 && p.pieces[0].want.probs == probs + 52 * 3 && p.pieces[0].want.inactive == inact + 52);
  CHECK(p.pieces[0].last && p.nnz == 48 * 3 && p.set_nodes == 3);
  p = plan_batch(q, 96, O);
  CHECK(p.kind == Want::rows && p.pieces.size() == 1 && p.nnz == 0 && !p.pieces[0].want.nodes);  // no set request rides in a dense batch
  p = plan_batch(q, 96, O);
  CHECK(p.kind == Want::set && p.pieces.size() == 1 && p.rows == 7);  // ... and no bit-mask request in a set batch
  p = plan_batch(q, 96, O);
  CHECK(p.kind == Want::rows_behind_bits && p.pieces.size() == 1 && !p.pieces[0].want.nodes);
  p = plan_batch(q, 96, O);
  CHECK(p.kind == Want::set && p.rows == 3 && q.empty());
  // raw set requests: the raw / spec rule on top, unchanged
  const SpliceRef spec = std::make_shared<const SpliceSpec>(SpliceSpec{{-1, 0, 1}, 13, 1, 1});
  Request raw = set_req(6, 20, a);
  raw.frames = Frames::raw_rows(x, spec, 20, 0);
  std::deque<Request> q2{raw, set_req(7, 5, a), raw};
  p = plan_batch(q2, 96, O);
  CHECK(p.kind == Want::set && p.raw && p.pieces.size() == 1 && p.raw_src.size() == 1 && p.segs.size() == 1 && p.nnz == 60);
  p = plan_batch(q2, 96, O);
  CHECK(p.kind == Want::set && !p.raw && p.pieces.size() == 1);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "rowptr") == 0) {
    V seg_rows, set_ptr, *into = &seg_rows;
    for (int i = 2; i < argc; ++i) {
      if (std::strcmp(argv[i], "/") == 0)
        into = &set_ptr;
      else
        into->push_back(std::atoi(argv[i]));
    }
    CHECK(seg_rows.size() == set_ptr.size() && !seg_rows.empty());
    for (int32_t v : sets::row_ptr(whole(seg_rows, set_ptr))) std::printf("%d ", v);
    std::printf("\n");
    return 0;
  }
  validator();
  covers();
  slices();
  server_plan();
  std::printf("sets ok\n");
  return 0;
}
