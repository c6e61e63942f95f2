// lists_union_check.cpp -- the host half of lazy output by lists over per-frame-group node unions (fdnn_lists_union.hpp),
// checked without a GPU: union_ref against a brute-force union and rank on random, empty, full, hostile, duplicated and
// descending lists, for g in {1, 2, 8} and row counts around the group seams; the work-item count against the grid bound;
// every index against the buffer sizes the header states (the buffers here are exactly that large: a write past one is the
// sanitizer's to find); and the shape rule.  Built with -fsanitize=address,undefined and run as a child process by
// tests/test_lazy_lists_union_host.py; exit status 0 = all cases hold.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "fdnn_lists_union.hpp"

using namespace fdnn;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

namespace {

constexpr int32_t kUntouched = -77;
int g_cases = 0;

struct Lists {
  std::vector<int32_t> row_ptr{0}, nodes;
  void add(const std::vector<int32_t> &row) {
    nodes.insert(nodes.end(), row.begin(), row.end());
    row_ptr.push_back(int32_t(nodes.size()));
  }
  int count() const { return int(row_ptr.size()) - 1; }
};

std::vector<int32_t> random_row(std::mt19937 &rng, int O, double share) {
  std::vector<int32_t> row;
  std::bernoulli_distribution pick(share);
  for (int v = 0; v < O; ++v)
    if (pick(rng)) row.push_back(v);
  return row;
}

// union_ref into exactly-sized buffers laid out by lunion::layout, against a brute force over std::set
void check_case(const Lists &l, int O, int g) {
  ++g_cases;
  const int count = l.count(), nnz = l.row_ptr.back();
  const lunion::Layout lay = lunion::layout(nnz, count, g);
  CHECK(lay.n_groups == (count + 32 * g - 1) / (32 * g));
  CHECK(lay.bound == nnz / 64 + lay.n_groups);
  CHECK(lay.pos == size_t(nnz) && lay.u_len == 2 * size_t(nnz) && lay.work == lay.u_len + size_t(lay.n_groups));
  CHECK(lay.counter == lay.work + 2 * size_t(lay.bound) && lay.words == lay.counter + 1);
  std::vector<int32_t> buf(lay.words, kUntouched);  // one buffer, as the context keeps it
  std::vector<int32_t> rp(l.row_ptr), nd(l.nodes);  // exactly sized copies
  const long long items = lunion::union_ref(rp.data(), nd.data(), count, nnz, O, g, buf.data() + lay.u_len, buf.data() + lay.u_nodes, buf.data() + lay.pos);
  CHECK(items <= lay.bound);
  for (size_t i = lay.work; i < lay.words; ++i) CHECK(buf[i] == kUntouched);  // the restatement keeps no work list
  long long want_items = 0;
  for (int q = 0; q < lay.n_groups; ++q) {
    const int r0 = q * 32 * g, r1 = std::min(count, r0 + 32 * g);
    const lunion::Range r = lunion::group_range(rp.data(), count, nnz, g, q);
    CHECK(r.b == rp[size_t(r0)] && r.e == rp[size_t(r1)]);  // well-formed row pointers: the clamp changes nothing
    std::set<int32_t> u;
    for (int i = r.b; i < r.e; ++i)
      if (nd[size_t(i)] >= 0 && nd[size_t(i)] < O) u.insert(nd[size_t(i)]);
    const std::vector<int32_t> sorted(u.begin(), u.end());
    const int32_t len = buf[lay.u_len + size_t(q)];
    CHECK(len == int32_t(sorted.size()) && len <= r.e - r.b);
    for (int j = 0; j < r.e - r.b; ++j) {
      const int32_t got = buf[lay.u_nodes + size_t(r.b) + size_t(j)];
      CHECK(j < len ? got == sorted[size_t(j)] : got == kUntouched);
    }
    for (int i = r.b; i < r.e; ++i) {
      const int32_t p = buf[lay.pos + size_t(i)], v = nd[size_t(i)];
      if (v < 0 || v >= O) {
        CHECK(p == -1);
      } else {
        CHECK(p >= 0 && p < len && sorted[size_t(p)] == v);
        // the work item that scores this entry is chunk p / 64 of group q: inside the group's items
        CHECK(p / 64 < (len + 63) / 64);
      }
    }
    want_items += (len + 63) / 64;
  }
  CHECK(items == want_items);
}

void all_shapes(const Lists &l, int O) {
  for (int g : {1, 2, 8}) check_case(l, O, g);
}

Lists random_lists(std::mt19937 &rng, int n, int O, double share) {
  Lists l;
  std::vector<int32_t> cur = random_row(rng, O, share);
  for (int r = 0; r < n; ++r) {
    if (r % 7 == 3)
      l.add({});  // empty rows among the others
    else
      l.add(cur);
    // a slowly changing set: a few nodes leave, a few arrive
    std::set<int32_t> s(cur.begin(), cur.end());
    for (int k = 0; k < 3; ++k) {
      if (!s.empty() && rng() % 2) s.erase(std::next(s.begin(), long(rng() % s.size())));
      s.insert(int32_t(rng() % uint32_t(O)));
    }
    cur.assign(s.begin(), s.end());
  }
  return l;
}

void shape_rule() {
  CHECK(lunion::shape_applies(2048, 8000, 2064, 2064));
  CHECK(lunion::shape_applies(256, 1000, 272, 272));
  CHECK(lunion::shape_applies(2048, lunion::kMaxNodes, 2064, 2064));
  CHECK(!lunion::shape_applies(2048, lunion::kMaxNodes + 1, 2064, 2064));  // the bitset's bound
  CHECK(!lunion::shape_applies(2064, 8000, 2080, 2080));                   // K > 2048: the tile's
  CHECK(!lunion::shape_applies(250, 1000, 272, 272));                      // K % 16
  CHECK(!lunion::shape_applies(256, 0, 272, 272));
  CHECK(lunion::group_tiles_of(0) == 0 && lunion::group_tiles_of(-1) == lunion::kDefaultGroupTiles);
  CHECK(lunion::kDefaultGroupTiles >= 1 && lunion::kDefaultGroupTiles <= lunion::kMaxGroupTiles);
  for (int g = 1; g <= lunion::kMaxGroupTiles; ++g) CHECK(lunion::group_tiles_of(g) == g);
  CHECK(lunion::group_tiles_of(9) == -1 && lunion::group_tiles_of(-2) == -1 && lunion::group_tiles_of(INT_MAX) == -1);
  CHECK(lunion::kMaxWords * lunion::kBitWord == lunion::kMaxNodes);
}

// a device list's row pointer is not validated: whatever it holds, a group's range stays inside [0, nnz] and union_ref
// (the kernel's statement) writes nothing outside the buffers
void hostile_row_ptr() {
  std::mt19937 rng(5);
  const int O = 300, count = 70, nnz = 900;
  std::vector<int32_t> nd(static_cast<size_t>(nnz), 0);
  for (auto &v : nd) v = int32_t(rng() % uint32_t(O + 20)) - 10;
  for (int round = 0; round < 50; ++round) {
    std::vector<int32_t> rp(size_t(count) + 1);
    for (auto &v : rp) v = int32_t(rng() % 3000) - 1000;
    if (round % 2) rp[0] = 0;
    for (int g : {1, 2, 8}) {
      const lunion::Layout lay = lunion::layout(nnz, count, g);
      std::vector<int32_t> buf(lay.words, kUntouched);
      for (int q = 0; q < lay.n_groups; ++q) {
        const lunion::Range r = lunion::group_range(rp.data(), count, nnz, g, q);
        CHECK(0 <= r.b && r.b <= r.e && r.e <= nnz);
      }
      lunion::union_ref(rp.data(), nd.data(), count, nnz, O, g, buf.data() + lay.u_len, buf.data() + lay.u_nodes, buf.data() + lay.pos);
      for (int q = 0; q < lay.n_groups; ++q) {
        const lunion::Range r = lunion::group_range(rp.data(), count, nnz, g, q);
        CHECK(buf[lay.u_len + size_t(q)] >= 0 && buf[lay.u_len + size_t(q)] <= r.e - r.b);
      }
    }
  }
}

}  // namespace

int main() {
  shape_rule();
  std::mt19937 rng(16);
  for (int n : {1, 31, 32, 33, 64, 65, 257}) {
    const int O = n == 257 ? 1000 : 251;
    all_shapes(random_lists(rng, n, O, 0.05), O);   // random, slowly changing, with empty rows
    all_shapes(random_lists(rng, n, O, 0.40), O);
    {  // a row listing every node, in the call's last group
      Lists l = random_lists(rng, n, O, 0.02);
      std::vector<int32_t> full(static_cast<size_t>(O), 0);
      for (int v = 0; v < O; ++v) full[size_t(v)] = v;
      l.row_ptr.pop_back();
      l.nodes.resize(size_t(l.row_ptr.back()));
      l.add(full);
      all_shapes(l, O);
    }
    {  // only empty rows: every group has u_len 0, no work item
      Lists l;
      for (int r = 0; r < n; ++r) l.add({});
      all_shapes(l, O);
    }
    if (n > 32) {  // rows 32 .. 63 empty: a whole group (g = 1) without entries between two that have some
      Lists l;
      for (int r = 0; r < n; ++r) l.add(r >= 32 && r < 64 ? std::vector<int32_t>{} : random_row(rng, O, 0.1));
      all_shapes(l, O);
    }
    {  // invalid nodes, duplicates and descending rows (what a device list may hold)
      Lists l = random_lists(rng, n, O, 0.10);
      for (size_t i = 0; i < l.nodes.size(); i += 5) l.nodes[i] = (i % 3 == 0) ? -1 : (i % 3 == 1) ? O : INT32_MAX;
      for (size_t i = 2; i + 1 < l.nodes.size(); i += 11) l.nodes[i] = l.nodes[i - 1];  // duplicates
      for (int r = 0; r < n; r += 4) std::reverse(l.nodes.begin() + l.row_ptr[size_t(r)], l.nodes.begin() + l.row_ptr[size_t(r) + 1]);
      if (!l.nodes.empty()) l.nodes.back() = INT32_MIN;
      all_shapes(l, O);
    }
  }
  {  // the widest layer the bitset takes: node kMaxNodes - 1 and node 0 in one union
    Lists l;
    l.add({0, lunion::kMaxNodes - 1});
    l.add({lunion::kMaxNodes - 1});
    all_shapes(l, lunion::kMaxNodes);
  }
  hostile_row_ptr();
  std::printf("lists union ok: %d cases\n", g_cases);
  return 0;
}
