// pair_check.cpp -- the pair-saturation arithmetic every kernel shares (fdnn_pair.hpp), checked without a GPU: the
// correction against the definition (dnn.cc:337-340) for every activation pair, the screen predicate against the
// correction, both entry decoders against the code that packs the entries, the accumulator slot against the MFMA's D
// layout, and the entry cursor over hand-made groups.  Built with -fsanitize=address,undefined (the cursor's reads past a
// group's last entry are the sanitizer's to find: every list below is an exactly sized heap block) and run as a child
// process by tests/test_pair_host.py; exit status 0 = all cases hold.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "fdnn_lists.hpp"  // lists::pack_pair
#include "fdnn_model.hpp"  // FixEntry
#include "fdnn_pair.hpp"

using namespace fdnn;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

namespace {

// the definition, on its own: the int32 sum of the two u8 x s8 products, saturated to int16, minus the sum
int excess_by_definition(int a0, int a1, int w0, int w1) {
  const int32_t sum = int32_t(uint8_t(a0)) * int32_t(int8_t(w0)) + int32_t(uint8_t(a1)) * int32_t(int8_t(w1));
  const int32_t sat = std::max<int32_t>(INT16_MIN, std::min<int32_t>(INT16_MAX, sum));
  return sat - sum;
}

long long all_activations(int w0, int w1) {
  const PairScreen sc = pair_screen(w0, w1);
  long long fired = 0;
  for (int a0 = 0; a0 < 256; ++a0)
    for (int a1 = 0; a1 < 256; ++a1) {
      const uint32_t staged = uint32_t(a0 ^ 0x80) | uint32_t(a1 ^ 0x80) << 8;  // s8 = u8 - 128: bit 7 flipped
      const int want = excess_by_definition(a0, a1, w0, w1);
      if (pair_excess(staged, w0, w1) != want || pair_fires(int(staged), sc) != (want != 0)) {
        std::fprintf(stderr, "a = (%d, %d), w = (%d, %d): excess %d, definition %d, screen %d\n", a0, a1, w0, w1, pair_excess(staged, w0, w1),
                     want, int(pair_fires(int(staged), sc)));
        std::exit(1);
      }
      fired += want != 0;
    }
  return fired;
}

void arithmetic() {
  std::vector<int> ws;
  for (int m : {0, 1, 61, 64, 122, 127, 128})
    for (int s : {1, -1})
      if (s * m >= -128 && s * m <= 127 && std::find(ws.begin(), ws.end(), s * m) == ws.end()) ws.push_back(s * m);
  CHECK(ws.size() == 12);  // 0, -128 once; 1, 61, 64, 122, 127 with both signs
  long long fired = 0;
  for (int w0 : ws)
    for (int w1 : ws) fired += all_activations(w0, w1);
  CHECK(all_activations(0, 0) == 0 && all_activations(64, 64) == 0);  // 255 * 128 = 32640: cannot saturate
  CHECK(all_activations(127, 127) > 0 && all_activations(-128, -128) > 0 && all_activations(127, -128) == 0);
  std::mt19937 rng(20337);
  std::uniform_int_distribution<int> w(-128, 127);
  for (int i = 0; i < 1000; ++i) {
    const int w0 = w(rng), w1 = w(rng);
    fired += all_activations(w0, w1);
  }
  CHECK(fired > 0);
}

void decoders() {
  for (int k : {0, 65534})
    for (int w0 : {-128, 127})
      for (int w1 : {-128, 127})
        for (int32_t node : {0, INT32_MAX}) {
          const FixEntry e{uint16_t(k), int8_t(w0), int8_t(w1), node};
          uint64_t raw;
          static_assert(sizeof raw == sizeof e, "a FixEntry is one 64-bit word");
          std::memcpy(&raw, &e, sizeof raw);
          const PairEntry a = decode_entry(raw);
          CHECK(a.k == k && a.w0 == w0 && a.w1 == w1 && a.node == node && entry_k(raw) == k);
          const PairEntry b = decode_pair(lists::pack_pair(e));
          CHECK(b.k == k && b.w0 == w0 && b.w1 == w1);
        }
}

// the inverse of "row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)", tile mi holding nodes 32 mi .. 32 mi + 31
void slots() {
  int seen[64] = {};
  for (int mi = 0; mi < 2; ++mi)
    for (int reg = 0; reg < 16; ++reg)
      for (int half = 0; half < 2; ++half) {
        const int node = 32 * mi + (reg & 3) + 8 * (reg >> 2) + 4 * half;
        CHECK(node >= 0 && node < 64);
        const AccSlot s = acc_slot(node);
        CHECK(s.idx == 16 * mi + reg && s.half == half);
        ++seen[node];
      }
  for (int n = 0; n < 64; ++n) CHECK(seen[n] == 1);
}

uint64_t word(int k, int w0, int w1, int32_t node) {
  const FixEntry e{uint16_t(k), int8_t(w0), int8_t(w1), node};
  uint64_t raw;
  std::memcpy(&raw, &e, sizeof raw);
  return raw;
}

// Three 64-node groups: none, one entry, five entries with repeated k.  Each group is walked over a list that ENDS with
// the group (an exactly sized block), once entry by entry and once as the kernels do, k-step by k-step.
void cursor() {
  const std::vector<uint64_t> all = {word(130, 127, 127, 70),                                                      // group 1
                                     word(0, -128, -128, 128), word(0, 127, 126, 191), word(126, 127, 127, 130),   // group 2
                                     word(128, -128, -127, 128), word(65534, 127, 127, 191)};
  const int32_t fix_grp[4] = {0, 0, 1, 6};
  for (int grp = 0; grp < 3; ++grp) {
    const int b = fix_grp[grp], end = fix_grp[grp + 1];
    uint64_t *ent = new uint64_t[size_t(end)];  // entries [0, end): index `end` is past the block
    std::copy(all.begin(), all.begin() + end, ent);
    const FixCursor closed = {0, 0, INT_MAX, fix_entries(ent), 0, 0};
    FixCursor fx = fix_open(closed, fix_grp, grp);
    CHECK(fx.e == b && fx.end == end);
    for (int e = b; e < end; ++e) {
      CHECK(fx.e == e && fx.raw == ent[e] && fx.k_next == entry_k(ent[e]));
      CHECK(e + 1 >= end || fx.raw_nxt == ent[e + 1]);
      fx = fix_advance(fx);
    }
    CHECK(fx.e == end && fx.k_next == INT_MAX);
    // the kernels' loop: k-steps of 128 columns, `while (k_next < (kt + 1) * BK)`
    fx = fix_open(closed, fix_grp, grp);
    int e = b;
    for (int kt = 0; kt < 65536 / 128; ++kt)
      while (fx.k_next < (kt + 1) * 128) {
        CHECK(e < end && fx.raw == ent[e] && entry_k(fx.raw) / 128 == kt);
        ++e;
        fx = fix_advance(fx);
      }
    CHECK(e == end && fx.k_next == INT_MAX);
    delete[] ent;
  }
}

}  // namespace

int main() {
  arithmetic();
  decoders();
  slots();
  cursor();
  std::printf("pair ok\n");
  return 0;
}
