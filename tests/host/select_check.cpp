// select_check.cpp -- the kernel selection (fdnn_select.hpp) checked without a GPU.  Built with -fsanitize=address,undefined
// and run as a child process by tests/test_select_host.py (argument: the recorded table); exit status 0 = all cases hold.
//  1. select_table.txt: what the selection answered BEFORE it was gathered into the header, recorded from the library's
//     objects of that commit -- for a list of layer shapes and switch settings, every frame count in 1 .. 70 000 at which
//     any part of the choice changes, and the choice from there on.  The header reproduces it line by line.
//  2. For every row of it, "will the hidden layers chain" and "will the output layer fuse" -- the questions frame_chunks
//     and the scoring loop ask beforehand -- equal what the pass planner does.
//  3. The frame-tile statement the dispatch ledger's exclusions rest on (tests/dispatch_ledger.py: EXCLUDED).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "fdnn_select.hpp"
#include "select_cases.hpp"  // Setting, kSettings, kMaxFrames, tuning_of

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

// ---------------------------------------------------------------------------------------- the table's cases and driver
struct Shape {
  const char *name;
  int rows, rows_pad, K;
  bool fastdiv, has_fix, output;
};
const Shape kShapes[] = {
    {"hid.256x256", 256, 256, 256, true, false, false},
    {"hid.2048x2048", 2048, 2048, 2048, true, false, false},
    {"hid.2048x2048.fix", 2048, 2048, 2048, true, true, false},
    {"hid.2304x2304", 2304, 2304, 2304, true, false, false},
    {"hid.2048x2048.tdiv", 2048, 2048, 2048, false, false, false},
    {"out.8000x2048", 8000, 8192, 2048, true, false, true},
    {"out.8000x2048.fix", 8000, 8192, 2048, true, true, true},
    {"out.8001x2048", 8001, 8192, 2048, true, false, true},
    {"out.33024x2304", 33024, 33024, 2304, true, false, true},  // 129 node tiles
    {"out.8000x2048.tdiv", 8000, 8192, 2048, false, true, true},
};
const int kHiddenDepths[] = {1, 6, 9};  // int8 hidden layers of the net (9: more than one chained launch holds)
const int kL0Dims[] = {64, 432, 496, 500, 2048};
constexpr int kL0Hidden = 2048;

// what is chosen at one frame count: the part that is constant over long runs of n as text, what moves with every tile
// (padded frame counts, the chain's tile) as two sums over the run
struct Row {
  const char *what = "";  // the form / the plan / layer 0's kind
  int v[6] = {0, 0, 0, 0, 0, 0};
  unsigned a = 0, b = 0;
  bool same_key(const Row &o) const { return std::strcmp(what, o.what) == 0 && std::equal(v, v + 6, o.v); }
};

template <class Fn>
void emit_runs(std::string &out, const std::string &section, int n_max, Fn row_at) {
  out += "[" + section + "]\n";
  Row run = row_at(1);
  int start = 1;
  for (int n = 2; n <= n_max + 1; ++n) {
    Row r;
    if (n <= n_max) r = row_at(n);
    if (n > n_max || !r.same_key(run)) {
      out += std::to_string(start) + ": " + run.what;
      for (int v : run.v) out += " " + std::to_string(v);
      out += " | " + std::to_string(run.a) + " " + std::to_string(run.b) + "\n";
      run = r;
      start = n;
    } else {
      run.a += r.a;
      run.b += r.b;
    }
  }
}

// E: configure(setting), layer(shape, setting, n), hidden(shape, depth, setting, n), l0(D, fma, kind, taps, n) -> Row.
// fuse_off: the sections recorded in a process with FDNN_FUSE_NORM=0 (the library reads it once)
template <class E>
void emit_table(E &e, bool fuse_off, std::string &out) {
  for (const Setting &s : kSettings) {
    if (s.fuse_off != fuse_off) continue;
    e.configure(s);
    // a switch is recorded with the decisions it bears on: chain with the pass, pp with hidden layers, ppo and masks with output layers
    const bool pass_only = s.chain_mode >= 0, hidden_only = s.pp_mode >= 0, output_only = s.ppo_mode >= 0 || s.byte_mask || s.bit_mask;
    for (const Shape &l : kShapes) {
      if (!pass_only && !(l.output ? hidden_only : output_only))
        emit_runs(out, std::string("layer ") + l.name + " " + s.name, kMaxFrames, [&](int n) { return e.layer(l, s, n); });
      if (l.output || hidden_only || output_only || s.fuse_off) continue;
      for (int depth : kHiddenDepths)
        emit_runs(out, std::string("hidden ") + l.name + " x" + std::to_string(depth) + " " + s.name, kMaxFrames, [&](int n) { return e.hidden(l, depth, s, n); });
    }
  }
  if (fuse_off) return;
  for (int D : kL0Dims)
    for (int fma = 0; fma < 2; ++fma)
      for (int kind = 0; kind <= 4; ++kind)
        for (int taps = 0; taps < 2; ++taps)
          emit_runs(out, "l0 D" + std::to_string(D) + (fma ? " fma" : " canonical") + " kind" + std::to_string(kind) + (taps ? " taps" : " prod"), kMaxFrames,
                    [&](int n) { return e.l0(D, fma != 0, kind, taps != 0, n); });
}

// an int8 layer: frame tile, node tile, tiled shape (GemmShape, else -1), small hidden tile (1 / 2, else 0), fused, mask as bits
Row layer_row(const char *form, int ft, int nt, int shape, int ntm, bool fused, bool bits) { return {form, {ft, nt, shape, ntm, fused ? 1 : 0, bits ? 1 : 0}}; }
// layer 0: tile, split tile width, fix-list variant {blocks, threads, lanes per output}
Row l0_row(const char *kind, int tile, int wn, int nb, int thr, int lpo) { return {kind, {tile, wn, nb, thr, lpo, 0}}; }

// ------------------------------------------------------------------------------------------ the header under the driver
struct HeaderEval {
  Tuning t;
  Device dev;  // 256 CUs: what the recording process, without a GPU, assumed

  void configure(const Setting &s) { t = tuning_of(s); }
  static LayerShape shape(const Shape &l) { return {l.rows, l.rows_pad, l.K, l.fastdiv, l.has_fix, l.output}; }
  static LayerCall call(const Shape &l, const Setting &s, int n) {
    LayerCall c{n};
    c.tap_acc = s.taps;
    c.tap_logit = s.taps && l.output;
    c.byte_mask = s.byte_mask && l.output;
    c.bit_mask = s.bit_mask && l.output;
    return c;
  }
  Row layer(const Shape &l, const Setting &s, int n) {
    const LayerCall c = call(l, s, n);
    const LayerChoice ch = choose_layer(shape(l), c, t);
    CHECK(ch.n_pad == round_up_to(n, ch.frame_tile) && ch.n_pad >= n);
    if (l.output) {
      // the question the scoring loop asks beforehand (output_will_fuse: a dense or byte-mask call without taps, whatever the
      // context) has the planner's answer
      LayerCall q{n};
      q.byte_mask = c.byte_mask || c.bit_mask;
      if (!s.taps) CHECK(choose_layer(shape(l), q, t).fused == ch.fused);
      CHECK(!ch.fused || (ch.form != Form::small && !s.taps && !s.fuse_off));
      CHECK((ch.form == Form::ppo) <= ch.fused);
      q.may_fuse = false;
      CHECK(!choose_layer(shape(l), q, t).fused);
    }
    const char *form = ch.form == Form::small ? "small" : ch.form == Form::tiled ? "tiled" : ch.form == Form::pp ? "pp" : "ppo";
    Row r = layer_row(form, ch.frame_tile, ch.node_tile, ch.form == Form::tiled ? int(ch.shape) : -1, ch.form == Form::small && !l.output ? ch.small_ntm : 0, ch.fused,
                      ch.mask_bits);
    r.a = unsigned(ch.n_pad);
    r.b = l.output ? unsigned(ch.partial_ld) : 0;
    return r;
  }
  Row hidden(const Shape &l, int depth, const Setting &s, int n) {
    auto at = [&](int) { return shape(l); };
    const HiddenPlan p = plan_hidden(depth, at, n, !s.taps, t, dev);
    // the question frame_chunks asks beforehand (hidden_layers_chain: no taps, a healthy context) has the planner's answer
    if (!s.taps) CHECK(plan_hidden(depth, at, n, true, t, dev).chain == p.chain);
    CHECK(!plan_hidden(depth, at, n, false, t, dev).chain);
    if (p.chain) {
      CHECK(p.n_pad == round_up_to(n, p.frame_tile) && (p.frame_tile == 256 || p.frame_tile == 320));
      int covered = 0;
      for (int q0 = 0; q0 < depth; q0 += kMaxChainLayers) covered += chain_segment(depth, q0);
      CHECK(covered == depth);
      // one layer that differs, or lacks the validated division, and nothing chains
      auto odd = [&](int i) {
        LayerShape x = shape(l);
        if (i == depth - 1) x.rows -= 1;
        return x;
      };
      auto slow = [&](int i) {
        LayerShape x = shape(l);
        if (i == 1) x.fastdiv = false;
        return x;
      };
      CHECK(!plan_hidden(depth, odd, n, true, t, dev).chain && !plan_hidden(depth, slow, n, true, t, dev).chain);
    }
    Row r;
    r.what = p.chain ? "chain" : "per-layer";
    r.a = unsigned(p.chain ? p.frame_tile : 0);
    return r;
  }
  Row l0(int D, bool fma, int kind, bool taps, int n) {
    const L0Call c{D, kL0Hidden, kL0Hidden, n, n, fma, kind, taps, true, true, l0_split_ok(D, kL0Hidden)};
    const L0Choice ch = choose_l0(c, t);
    static const char *const names[] = {"mfma", "small", "split", "screened", "chain", "tile64"};
    return l0_row(names[int(ch.kind)], ch.tile, ch.split_wn, ch.fix_nb, ch.fix_threads, ch.fix_lpo);
  }
};

void check_table(const char *path) {
  std::ifstream f(path);
  CHECK(f.good());
  std::stringstream want;
  want << f.rdbuf();
  HeaderEval e;
  std::string got;
  emit_table(e, false, got);
  emit_table(e, true, got);
  if (got != want.str()) {
    std::istringstream a(got), b(want.str());
    std::string la, lb, section;
    int line = 0;
    while (true) {
      const bool ha = bool(std::getline(a, la)), hb = bool(std::getline(b, lb));
      ++line;
      if (!ha && !hb) break;
      if (ha && la[0] == '[') section = la;
      if (!ha || !hb || la != lb) {
        std::fprintf(stderr, "select table line %d, %s:\n  header:   %s\n  recorded: %s\n", line, section.c_str(), ha ? la.c_str() : "<end>", hb ? lb.c_str() : "<end>");
        break;
      }
    }
    std::exit(1);
  }
}

// The exclusions of the hidden-layer forms of the four-wave 128-frame shapes (tests/dispatch_ledger.py) rest on a statement
// about frame_tile: its cost model returns 128 only for layers of 129 node tiles or more (and nothing but 128, 256 or 320).
// Every width the loader accepts (2^19 nodes = 2048 node tiles), every frame count up to 392 + 100 345 / mt; beyond that no
// rounding can help the 128-frame tiles: cost128 >= 465 * mt * n / 65 536 and cost320 <= mt * n / 256 + 1.25 * mt + 320, so
// 128 can undercut 320 only for n < 392 + 100 345 / mt.
void check_frame_tile_exclusion_argument() {
  const Tuning t;
  int lowest = 0;
  for (int mt = 1; mt <= 2048; ++mt) {
    bool model_128 = false;
    for (int n = 1; n <= 392 + 100345 / mt + 1; ++n) {
      bool from_model = false;
      const int ft = frame_tile(256 * mt, n, t, &from_model);
      CHECK(ft == 32 || ft == 64 || ft == 128 || ft == 256 || ft == 320);
      CHECK(!from_model || ft >= 128);
      model_128 = model_128 || (ft == 128 && from_model);
    }
    if (model_128) {
      if (!lowest) lowest = mt;
      CHECK(mt >= 129);
    }
  }
  CHECK(lowest == 129);
  // and the model is the function the ledger's wide-output cases meet on the device: 129 node tiles, 321 .. 384 frames
  const int n[4] = {320, 321, 384, 385}, want[4] = {320, 128, 128, 256};
  for (int i = 0; i < 4; ++i) {
    bool from_model = false;
    CHECK(frame_tile(256 * 129, n[i], t, &from_model) == want[i] && from_model);
  }
}

// "forced mode, else the environment's; forced minimum, else the environment's": the one resolution behind chain, pp and ppo
void check_mode_resolution() {
  CHECK(resolve_mode(-1, 0, -1, 9800).mode == -1 && resolve_mode(-1, 0, -1, 9800).min_frames == 9800 && !resolve_mode(-1, 0, -1, 9800).forced_on);
  CHECK(resolve_mode(-1, 700, 1, 9800).min_frames == 9800);  // a minimum without a forced mode is not forced
  CHECK(resolve_mode(1, 700, 0, 9800).mode == 1 && resolve_mode(1, 700, 0, 9800).min_frames == 700 && resolve_mode(1, 700, 0, 9800).forced_on);
  CHECK(resolve_mode(0, 0, 1, 4000).mode == 0 && resolve_mode(0, 0, 1, 4000).min_frames == 4000);
  CHECK(resolve_mode(-1, 0, 1, 4000).mode == 1 && !resolve_mode(-1, 0, 1, 4000).forced_on);  // FDNN_CHAIN=1 is not the override's 1
  // the chain's idle-CU test follows the device: 304 CUs, 2048-wide layers, 10 240 frames = 256 tiles, 48 CUs idle
  const Tuning t;
  CHECK(!chain_ok(2048, 2048, 10240, 6, t, Device{256}) && chain_ok(2048, 2048, 10240, 6, t, Device{304}));
}

}  // namespace

int main(int argc, char **argv) {
  CHECK(argc == 2);
  check_mode_resolution();
  check_frame_tile_exclusion_argument();
  check_table(argv[1]);
  std::printf("select ok\n");
  return 0;
}
