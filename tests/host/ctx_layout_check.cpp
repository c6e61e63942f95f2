// ctx_layout_check.cpp -- the sizes of a context's scratch buffers (fdnn_ctx_layout.hpp) checked without a GPU.  Built with
// -fsanitize=address,undefined and run as a child process by tests/test_ctx_layout_host.py (argument: the recorded table);
// exit status 0 = all cases hold.
//  1. ctx_layout_table.txt: every count make_ctx computed BEFORE the sizes were gathered into the header, recorded from that
//     commit's expressions for the suite's net shapes and a list of frame counts.  The header reproduces it line by line.
//  2. For the same shapes, every frame count and switch setting of the selection sweep (select_cases.hpp) and a list of
//     forced tiles: whatever choose_l0, plan_hidden and choose_layer choose, the elements the launch indexes in each context
//     buffer (the header's extent functions, read off the kernels) number no more than the layout holds.
//  3. --seed K: the same check with one known fault planted in the layout (layout_of); the test runs them all.  Seeds 1, 2, 4
//     and 5 must fail.  Seed 3, the chain's "+ 2 tiles" removed, passes: a chained launch touches n_pad / FT counters per
//     layer (fdnn_chain.hip:111-119, :524), FT >= 256, and floor((cap + 320) / 256) >= ceil(n / 256) already -- the two
//     tiles are slack that no launch reaches.  Seed 5 drops the 320 frames as well and is caught.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "fdnn_ctx_layout.hpp"
#include "select_cases.hpp"

using namespace fdnn;
using namespace fdnn::sel;
using namespace select_cases;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

namespace {

struct Net {
  const char *name;
  int in_dim, hidden, n_hidden, out_dim;  // n_hidden: layer 0 + the int8 hidden layers
};
const Net kNets[] = {
    {"tiny", 432, 64, 3, 100},  // tests/golden/tiny.npz
    {"432.3x256.1000", 432, 256, 3, 1000},
    {"432.3x128.200", 432, 128, 3, 200},
    {"432.7x2048.8000", 432, 2048, 7, 8000},
    {"432.7x2048.8001", 432, 2048, 7, 8001},
    {"40.7x2048.8000", 40, 2048, 7, 8000},    // input widths outside the int8 screening's 64 .. 496
    {"500.7x2048.8000", 500, 2048, 7, 8000},
    {"432.3x144.40", 432, 144, 3, 40},        // hidden widths that are no multiple of 128: with the screening planes,
    {"432.3x200.300", 432, 200, 3, 300},      // and (200 % 16 != 0) without
    {"432.7x2000.8000", 432, 2000, 7, 8000},
    {"432.10x256.300", 432, 256, 10, 300},    // nine int8 hidden layers: a chained launch of kMaxChainLayers and one more
};
const int kTableFrames[] = {0, 1, 63, 64, 65, 127, 128, 129, 559, 560, 700, 1400, 4097, 9800, 10000, 10240, 20480};

int up(int v, int a) { return (v + a - 1) / a * a; }
int l0_chunk_rows(int D) {  // fdnn_l0.hip
  const int J = D / 4, p12 = (J + 11) / 12 * 12, p16 = (J + 15) / 16 * 16;
  return p12 <= p16 ? 12 : 16;
}
int rows_pad(int rows) { return up(rows, kRowPad); }  // fdnn_model.cpp
CtxShape shape_of(const Net &net, int n, bool lean, int tn, int list_cap) {
  return {net.in_dim, net.hidden, net.out_dim, std::max(rows_pad(net.hidden), rows_pad(net.out_dim)), up(net.in_dim / 4, l0_chunk_rows(net.in_dim)),
          up(net.hidden, 128), l0_split_ok(net.in_dim, net.hidden), tn, list_cap, lean, n};
}

// --seed K: a fault planted in the layout before it is checked; 0 = none
int g_seed = 0;
CtxLayout layout_of(const CtxShape &s) {
  CtxLayout l = ctx_layout(s);
  const size_t np = size_t(l.cap), npt = np + kMaxFrameTile, mt = size_t(s.max_rows_pad / 256);
  switch (g_seed) {
    case 1:  // the + kMaxFrameTile slack dropped
      l.act = np * l.act_ld;
      l.partial = np * (s.max_rows_pad / kPartialNodes);
      l.fuse_s = np * mt;
      break;
    case 2: l.fuse_cnt /= 2; break;                                 // half the fused counter words
    case 3: l.chain_done = (npt / 256) * kMaxChainLayers; break;    // the + 2 tiles of the chain sizing removed: NOT a shortfall, see main
    case 5: l.chain_done = (np / 256) * kMaxChainLayers; break;     // ... and its tile of slack frames too
    case 4:                                                         // xt_ld a multiple of 64
      l.xt_ld = up(l.cap, 64);
      l.xt = 4 * size_t(s.l0_j_pad) * l.xt_ld;
      if (s.split) l.xd = l0_split_plane_bytes(s.in_dim, l.xt_ld), l.xstat = 3 * size_t(l.xt_ld);
      break;
    default: break;
  }
  return l;
}

// ------------------------------------------------------------------------------------------------ 1. sizes unchanged
std::string table() {
  std::string out;
  for (const Net &net : kNets)
    for (int lean = 0; lean < 2; ++lean)
      for (int tn : {64, 128})
        for (int list_cap : {0, 1000})
          for (int n : kTableFrames) {
            const CtxLayout l = ctx_layout(shape_of(net, n, lean != 0, tn, list_cap));
            char head[160];
            std::snprintf(head, sizeof(head), "%s %s tn%d cap%d n%d:", net.name, lean ? "lean" : "full", tn, list_cap, n);
            out += head;
            for (int v : {l.cap, l.act_ld, l.xt_ld, l.glist_cap}) out += " " + std::to_string(v);
            for (size_t v : {l.x, l.xt, l.scr_count, l.scr_list, l.xd, l.xstat, l.glist_count, l.l0park, l.act, l.out, l.partial, l.mask, l.mask_bits,
                             l.fuse_s, l.fuse_cnt, l.fuse_flag, l.chain_ctl, l.chain_done, l.mask_pin, l.out_pin})
              out += " " + std::to_string(v);
            out += "\n";
          }
  return out;
}

void check_table(const char *path) {
  std::ifstream f(path);
  CHECK(f.good());
  std::stringstream want;
  want << f.rdbuf();
  const std::string got = table();
  if (got == want.str()) return;
  std::istringstream a(got), b(want.str());
  std::string la, lb;
  for (int line = 1;; ++line) {
    const bool ha = bool(std::getline(a, la)), hb = bool(std::getline(b, lb));
    if (!ha && !hb) break;
    if (!ha || !hb || la != lb) {
      std::fprintf(stderr, "layout table line %d:\n  header:   %s\n  recorded: %s\n", line, ha ? la.c_str() : "<end>", hb ? lb.c_str() : "<end>");
      break;
    }
  }
  std::exit(1);
}

// ---------------------------------------------------------------------------- 2. sizes cover what can be launched
long g_cases = 0;
struct Where {
  const char *net, *setting, *forced;
  int n;
} g_at;
#define COVERS(extent, count)                                                                                                        \
  do {                                                                                                                               \
    if (!(size_t(extent) <= size_t(count))) {                                                                                        \
      std::fprintf(stderr, "%s:%d: %s = %zu exceeds %s = %zu (net %s, %d frames, setting %s, %s)\n", __FILE__, __LINE__, #extent, size_t(extent), \
                   #count, size_t(count), g_at.net, g_at.n, g_at.setting, g_at.forced);                                              \
      std::exit(1);                                                                                                                  \
    }                                                                                                                                \
  } while (0)

// what the measurement switches can force beyond the sweep's settings: tiles of the int8 layers, of the chain, of layer 0
struct Forced {
  const char *name;
  int frame_tile, node_tile, small_ntm, chain_tile, l0_screen_wfr, l0s_wn;
};
const Forced kForced[] = {
    {"unforced", 0, 0, 0, 0, 4, 0},      {"ft32", 32, 0, 0, 0, 4, 0},         {"ft64", 64, 0, 0, 0, 4, 0},       {"ft128.nt128", 128, 128, 0, 0, 4, 0},
    {"ft256.nt256", 256, 256, 0, 0, 4, 0}, {"ft320", 320, 0, 0, 0, 4, 0},      {"ntm1.chain256", 0, 0, 1, 256, 2, 1}, {"ntm2.chain320", 0, 0, 2, 320, 4, 2},
};

LayerShape int8_layer(const Net &net, bool output) {
  const int rows = output ? net.out_dim : net.hidden, K = up(net.hidden, kColPad);
  return {rows, rows_pad(rows), K, true, false, output};
}

enum Part { kL0 = 1, kHidden = 2, kOutput = 4 };
void check_launches(const Net &net, const Setting &s, const Forced &f, const Tuning &t, int n, int parts) {
  if (g_seed == 3 || g_seed == 5) parts &= kHidden;  // (these two touch the chain's counters only)
  g_at = {net.name, s.name, f.name, n};
  const CtxShape cs = shape_of(net, n, false, t.l0_chain_tn, 0);
  const CtxLayout l = layout_of(cs);
  CHECK(l.cap == up(std::max(n, 1), 64));
  // layer 0: both flavours, every requested kind
  for (int fma = 0; fma < 2 && (parts & kL0); ++fma)
    for (int kind = 0; kind <= 4; ++kind) {
      const L0Call c{net.in_dim, net.hidden, cs.l0_h_ld, n, n, fma != 0, kind, s.taps, true, true, cs.split};
      const L0Extent e = l0_extent(choose_l0(c, t), net.in_dim, net.hidden, cs.l0_h_ld, cs.l0_j_pad, n, l.act_ld, l.xt_ld, l.glist_cap);
      COVERS(e.act, l.act);
      COVERS(e.cols, l.xt_ld);
      COVERS(e.xt, l.xt);
      COVERS(e.l0park, l.l0park);
      COVERS(e.scr_count, l.scr_count);
      COVERS(e.scr_list, l.scr_list);
      COVERS(e.xd, l.xd);
      COVERS(e.xstat, l.xstat);
      COVERS(e.glist, l.glist_cap);
      COVERS(e.glist_count, l.glist_count);
      ++g_cases;
    }
  // the hidden layers: one chained launch per kMaxChainLayers layers, or a launch per layer
  const int n_hid = net.n_hidden - 1;
  const LayerShape hid = int8_layer(net, false);
  const HiddenPlan plan = plan_hidden(n_hid, [&](int) { return hid; }, n, !s.taps, t, Device{});
  if (plan.chain && (parts & kHidden)) {
    for (int q0 = 0; q0 < n_hid; q0 += kMaxChainLayers) {
      const ChainExtent e = chain_extent(plan, chain_segment(n_hid, q0), l.act_ld);
      COVERS(e.act, l.act);
      COVERS(e.ctl, l.chain_ctl);
      COVERS(e.done, l.chain_done);
    }
  }
  for (int qi : {0, n_hid - 1}) {  // (all hidden layers have one shape; also where the pass chains: a context whose chain counters are dirty goes layer by layer)
    if (qi < 0 || !(parts & kHidden)) continue;
    LayerCall c{n, qi};
    c.tap_acc = s.taps;
    const LayerExtent e = layer_extent(hid, choose_layer(hid, c, t), 0, n, l.act_ld);
    COVERS(e.act_in, l.act);
    COVERS(e.act_out, l.act);
  }
  g_cases += (parts & kHidden) ? 1 : 0;
  if (!(parts & kOutput)) return;
  // the output layer: the whole context, and sub-ranges [first, first + count) of it; dense and masked
  const LayerShape out = int8_layer(net, true);
  auto output_launch = [&](int first, int count, int mask, bool may_fuse) {
    if (first < 0 || count < 1 || first + count > n) return;
    LayerCall c{count};
    c.tap_acc = c.tap_logit = s.taps;
    c.byte_mask = mask == 1 || s.byte_mask;
    c.bit_mask = mask == 2 || s.bit_mask;
    c.may_fuse = may_fuse;
    const LayerExtent e = layer_extent(out, choose_layer(out, c, t), first, count, l.act_ld, c.byte_mask || c.bit_mask);
    COVERS(e.act_in, l.act);
    COVERS(e.partial, l.partial);
    COVERS(e.fuse_s, l.fuse_s);
    COVERS(e.fuse_cnt, l.fuse_cnt);
    COVERS(e.fuse_flag, l.fuse_flag);
    COVERS(e.mask_bits, l.mask_bits);
    ++g_cases;
  };
  for (int mask = 0; mask < 3; ++mask) output_launch(0, n, mask, true);
  output_launch(0, n, 0, false);  // (a context, process or model that may not fuse)
  const int sub[][2] = {{1, n - 1}, {n / 2, n - n / 2}, {n / 2, (n - n / 2) / 2}, {n - 1, 1}, {63, std::min(8, n - 63)}};
  for (const auto &r : sub)
    for (int mask : {0, 2}) output_launch(r[0], r[1], mask, true);
}

// A pooled context serves smaller batches at a larger cap: no count shrinks when cap grows, so the tight cap is the case to check.
void check_monotone() {
  for (const Net &net : kNets)
    for (int lean = 0; lean < 2; ++lean)
      for (int tn : {64, 128}) {
        CtxLayout prev = layout_of(shape_of(net, 1, lean != 0, tn, 0));
        for (int n = 65; n <= kMaxFrames + 64; n += 64) {
          const CtxLayout l = layout_of(shape_of(net, n, lean != 0, tn, 0));
          CHECK(l.cap == prev.cap + 64 && l.xt_ld >= prev.xt_ld && l.glist_cap >= prev.glist_cap && l.act_ld == prev.act_ld);
          CHECK(l.x >= prev.x && l.xt >= prev.xt && l.scr_count >= prev.scr_count && l.scr_list >= prev.scr_list && l.xd >= prev.xd && l.xstat >= prev.xstat);
          CHECK(l.glist_count >= prev.glist_count && l.l0park >= prev.l0park && l.act >= prev.act && l.out >= prev.out);
          CHECK(l.partial >= prev.partial && l.mask >= prev.mask && l.mask_bits >= prev.mask_bits && l.fuse_s >= prev.fuse_s && l.fuse_cnt >= prev.fuse_cnt);
          CHECK(l.fuse_flag >= prev.fuse_flag && l.chain_ctl >= prev.chain_ctl && l.chain_done >= prev.chain_done && l.mask_pin >= prev.mask_pin && l.out_pin >= prev.out_pin);
          prev = l;
        }
      }
}

// As select_check.cpp records them, a switch is checked with the decisions it bears on: chain with the pass, pp with the hidden
// layers, ppo, the soft-max switch and masks with the output layer (masks: every setting's output launches carry all three
// kinds); layer 0 sees taps and its node tile only.  The switches: every frame count 1 .. kMaxFrames.  Forced tiles, under the
// default switches: every frame count up to 4200 -- past the small-batch rules' thresholds -- then the three around every
// multiple of 32, between which neither the capacity nor any forced tile's padded frame count moves.
void check_cover() {
  check_monotone();
  for (const Net &net : kNets) {
    for (const Setting &s : kSettings) {
      if (s.byte_mask || s.bit_mask) continue;
      const bool defaults = &s == kSettings;
      const int parts = defaults || s.taps ? kL0 | kHidden | kOutput : (s.chain_mode >= 0 || s.pp_mode >= 0) ? kHidden : kOutput;
      for (int tn : {64, 128}) {
        if (tn == 128 && !defaults) continue;
        Tuning t = tuning_of(s);
        t.l0_chain_tn = tn;
        for (int n = 1; n <= kMaxFrames; ++n) check_launches(net, s, kForced[0], t, n, tn == 128 ? kL0 : parts);
      }
    }
    for (const Forced &f : kForced) {
      if (&f == kForced) continue;
      Tuning t = tuning_of(kSettings[0]);
      t.frame_tile = f.frame_tile;
      t.node_tile = f.node_tile;
      t.small_ntm = f.small_ntm;
      t.chain_tile = f.chain_tile;
      t.l0_screen_wfr = f.l0_screen_wfr;
      t.l0s_wn = f.l0s_wn;
      for (int n = 1; n <= kMaxFrames; ++n)
        if (n <= 4200 || n % 32 <= 1 || n % 32 == 31) check_launches(net, kSettings[0], f, t, n, kL0 | kHidden | kOutput);
    }
  }
}

// The scratch audit's table (kCtxScratch) against the layout: every counter field of CtxLayout -- the uint32 arrays make_ctx
// zeroes -- has a row in the table or an entry, with its reason, in the exemption list, and none has both; rows name distinct
// fields, and their word counts are the layout's for every shape.  sizeof(CtxLayout) pins the field list: whoever adds a
// field decides here whether it is a counter.  --names prints the table's names (tests/test_ctx_layout_host.py compares them
// with the library's).
void check_scratch_table(bool print) {
  static_assert(sizeof(CtxLayout) == 4 * sizeof(int) + 20 * sizeof(size_t), "CtxLayout changed: is the new field a counter array? (kCounters below)");
  size_t CtxLayout::*const kCounters[] = {&CtxLayout::scr_count, &CtxLayout::glist_count, &CtxLayout::fuse_cnt, &CtxLayout::fuse_flag,
                                          &CtxLayout::chain_ctl, &CtxLayout::chain_done};
  for (auto f : kCounters) {
    int rows = 0, exempt = 0;
    for (const CtxScratchRow &r : kCtxScratch) rows += r.words == f;
    for (const CtxScratchExempt &e : kCtxScratchExempt) exempt += e.words == f;
    CHECK(rows + exempt == 1);
  }
  int listed = 0;
  for (const CtxScratchRow &r : kCtxScratch) {
    CHECK(r.name && r.name[0]);
    bool known = false;
    for (auto f : kCounters) known = known || r.words == f;
    CHECK(known);
    for (const CtxScratchRow &o : kCtxScratch) CHECK(&o == &r || (o.words != r.words && std::strcmp(o.name, r.name) != 0));
    if (print) std::printf("%s%s", listed ? " " : "", r.name);
    ++listed;
  }
  if (print) std::printf("\n");
  for (const CtxScratchExempt &e : kCtxScratchExempt) CHECK(e.name && e.name[0] && e.zeroed_by && e.zeroed_by[0]);
  CHECK(listed == kCtxScratchCount && sizeof(kCounters) / sizeof(kCounters[0]) == kCtxScratchCount + sizeof(kCtxScratchExempt) / sizeof(kCtxScratchExempt[0]));
  CHECK(kCtxScratch[kScrCount].words == &CtxLayout::scr_count && kCtxScratch[kFuseCnt].words == &CtxLayout::fuse_cnt &&
        kCtxScratch[kFuseFlag].words == &CtxLayout::fuse_flag && kCtxScratch[kChainCtl].words == &CtxLayout::chain_ctl &&
        kCtxScratch[kChainDone].words == &CtxLayout::chain_done);
  // every listed buffer exists (non-empty) in every context, lean or not: the audit reads all of them
  for (const Net &net : kNets)
    for (int lean = 0; lean < 2; ++lean)
      for (int n : kTableFrames) {
        const CtxLayout l = ctx_layout(shape_of(net, n, lean != 0, 64, 0));
        for (const CtxScratchRow &r : kCtxScratch) CHECK(l.*(r.words) > 0);
      }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 2 && std::strcmp(argv[1], "--names") == 0) {
    check_scratch_table(true);
    return 0;
  }
  CHECK(argc == 2 || (argc == 4 && std::strcmp(argv[2], "--seed") == 0));
  if (argc == 4) g_seed = std::atoi(argv[3]);
  check_scratch_table(false);
  if (!g_seed) check_table(argv[1]);
  check_cover();
  std::printf("ctx layout ok: %ld launch cases\n", g_cases);
  return 0;
}
