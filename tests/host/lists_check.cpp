// lists_check.cpp -- the host half of lazy output by active-node lists (fdnn_lists.hpp), checked without a GPU: the
// validator on well-formed, random and hostile lists, and the per-node index of saturating pairs against a brute-force scan
// of the group-ordered entries.  Built with -fsanitize=address,undefined and run as a child process by
// tests/test_lazy_lists_host.py; exit status 0 = all cases hold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "fdnn_lists.hpp"

using namespace fdnn;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

namespace {

struct Lists {
  std::vector<int32_t> row_ptr{0}, nodes;
  void add(const std::vector<int32_t> &row) {
    nodes.insert(nodes.end(), row.begin(), row.end());
    row_ptr.push_back(int32_t(nodes.size()));
  }
  int count() const { return int(row_ptr.size()) - 1; }
  // exactly-sized copies: a read past either array is the sanitizer's to find
  int check(int O) const {
    std::vector<int32_t> rp(row_ptr), nd(nodes);
    return lists::check(rp.data(), nd.empty() ? nullptr : nd.data(), count(), O);
  }
};

std::vector<int32_t> random_row(std::mt19937 &rng, int O, double share) {
  std::vector<int32_t> row;
  std::bernoulli_distribution pick(share);
  for (int v = 0; v < O; ++v)
    if (pick(rng)) row.push_back(v);
  return row;
}

void validator() {
  const int O = 1000;
  std::mt19937 rng(7);
  {  // the shapes the contract names
    Lists l;
    l.add({});
    std::vector<int32_t> full(O);
    for (int v = 0; v < O; ++v) full[size_t(v)] = v;
    l.add(full);
    l.add({0});
    l.add({O - 1});
    l.add({});
    CHECK(l.check(O) == 0);
    CHECK(lists::check(l.row_ptr.data(), l.nodes.data(), 0, O) == 0);  // no rows: nothing to read
  }
  for (int round = 0; round < 200; ++round) {  // random well-formed lists, then one planted fault each
    Lists l;
    const int n = 1 + int(rng() % 40);
    for (int r = 0; r < n; ++r) l.add(random_row(rng, O, (r % 3 == 0) ? 0.0 : 0.05 * double(1 + rng() % 8)));
    CHECK(l.check(O) == 0);
    std::vector<int> nonempty, two;
    for (int r = 0; r < n; ++r) {
      if (l.row_ptr[size_t(r) + 1] > l.row_ptr[size_t(r)]) nonempty.push_back(r);
      if (l.row_ptr[size_t(r) + 1] > l.row_ptr[size_t(r)] + 1) two.push_back(r);
    }
    if (nonempty.empty()) continue;
    const int r1 = nonempty[rng() % nonempty.size()];
    const size_t at = size_t(l.row_ptr[size_t(r1)]) + rng() % size_t(l.row_ptr[size_t(r1) + 1] - l.row_ptr[size_t(r1)]);
    for (int32_t hostile : {-1, O, O + 12345, INT32_MIN, INT32_MAX}) {
      Lists b = l;
      b.nodes[at] = hostile;
      CHECK(b.check(O) == -(r1 + 1));
    }
    if (!two.empty()) {
      const int r2 = two[rng() % two.size()];
      const size_t p = size_t(l.row_ptr[size_t(r2)]);
      Lists dup = l, desc = l;
      dup.nodes[p + 1] = dup.nodes[p];  // a duplicate
      CHECK(dup.check(O) == -(r2 + 1));
      std::swap(desc.nodes[p], desc.nodes[p + 1]);  // a descending pair
      CHECK(desc.check(O) == -(r2 + 1));
    }
    {
      Lists b = l;
      b.row_ptr[0] = 1;  // row_ptr[0] != 0 answers as row 0
      CHECK(lists::check(b.row_ptr.data(), b.nodes.data(), n, O) == -1);
    }
    {  // a decreasing row_ptr: the row whose range runs backwards
      Lists b = l;
      b.row_ptr[size_t(r1) + 1] = b.row_ptr[size_t(r1)] - 1 - int32_t(rng() % 3);
      const int got = lists::check(b.row_ptr.data(), b.nodes.data(), n, O);
      CHECK(got == -(r1 + 1));
    }
    {  // a null node array is only good for empty rows
      CHECK(lists::check(l.row_ptr.data(), nullptr, n, O) == -(nonempty[0] + 1));
    }
  }
}

// rows nodes of `cols` columns; every pair (node, k) with risky(node, k) is an entry: the blob's layout (grouped by 64 nodes,
// sorted by k inside a group, ties in node order) against the per-node index
template <class Risky>
void fix_index(int rows, int cols, Risky risky) {
  const int rows_pad = (rows + 255) / 256 * 256;
  std::vector<FixEntry> ent;
  std::vector<int32_t> grp(size_t(rows_pad) / 64 + 1, 0);
  for (int g = 0; g < rows_pad / 64; ++g) {
    for (int k = 0; k < cols; k += 2)
      for (int node = 64 * g; node < std::min(rows, 64 * (g + 1)); ++node)
        if (risky(node, k)) ent.push_back(FixEntry{uint16_t(k), int8_t(node % 251 - 125), int8_t(-(k % 127)), node});
    grp[size_t(g) + 1] = int32_t(ent.size());
  }
  std::vector<FixEntry> exact(ent);  // (exactly sized; an empty list still has an address)
  exact.push_back(FixEntry{0, 0, 0, 0});
  std::vector<int32_t> off;
  std::vector<uint32_t> pairs;
  lists::build_node_fix_index(exact.data(), grp.data(), rows, rows_pad, &off, &pairs);
  CHECK(off.size() == size_t(rows) + 1 && off[0] == 0 && size_t(off[size_t(rows)]) == ent.size() && pairs.size() == ent.size());
  for (int node = 0; node < rows; ++node) {
    std::vector<uint32_t> want;  // brute force: every entry of this node, in list order
    for (const FixEntry &e : ent)
      if (e.node == node) want.push_back(lists::pack_pair(e));
    CHECK(off[size_t(node) + 1] - off[size_t(node)] == int32_t(want.size()));
    for (size_t i = 0; i < want.size(); ++i) {
      const uint32_t got = pairs[size_t(off[size_t(node)]) + i];
      CHECK(got == want[i]);
      CHECK(i == 0 || (got & 0xffffu) > (pairs[size_t(off[size_t(node)]) + i - 1] & 0xffffu));  // ascending k per node
      CHECK(int8_t(got >> 16) == int8_t(node % 251 - 125) && int8_t(got >> 24) == int8_t(-int((got & 0xffffu) % 127)));
    }
  }
}

void rebase() {
  const std::vector<int32_t> rp{0, 3, 3, 10, 11};
  std::vector<int32_t> out;
  lists::rebase_rows(rp.data(), 1, 3, &out);
  CHECK((out == std::vector<int32_t>{0, 0, 7, 8}));
  lists::rebase_rows(rp.data(), 0, 4, &out);
  CHECK(out == rp);
}

}  // namespace

int main() {
  validator();
  std::mt19937 rng(11);
  fix_index(200, 128, [](int, int) { return false; });                          // no entries
  fix_index(1000, 256, [&](int, int) { return rng() % 997 == 0; });             // a few
  fix_index(251, 64, [&](int node, int k) { return (node * 31 + k) % 5 == 0; });  // an odd width, a fifth of the pairs
  fix_index(300, 64, [](int, int) { return true; });                            // every pair risky
  rebase();
  std::printf("lists ok\n");
  return 0;
}
