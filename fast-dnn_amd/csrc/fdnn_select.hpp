// fdnn_select.hpp -- which kernel a layer launches: every rule of the selection as a pure function of plain structs (the
// layer's shape, what the call carries, the device's CU count, the switches).  No HIP in here: the launchers
// (fdnn_*.hip) map a choice to a kernel pointer and a grid, the runtime (fdnn_runtime.cpp) fills parameter structs from
// it and answers its callers' "will it chain / fuse" questions with the same functions, and tests/host/select_check.cpp
// runs the rules on the host.  The process's switches are read once, in fdnn_select.cpp.
#pragma once
#include <algorithm>
#include <atomic>

namespace fdnn {

constexpr int kMaxChainLayers = 8;  // hidden layers of one chained launch (QChainParams::layer)

// GEMM tile shapes of launch_qgemm (fdnn_gemm.hip), in the order of its switch; the last three are compiled only in a
// measurement build (-DFDNN_ABLATION), which takes them where FDNN_SMALL_BK is set
enum GemmShape { gs_tdiv, gs_ft32w1, gs_ft32, gs_ft64, gs_ft128nt128, gs_ft128bk128, gs_ft128, gs_ft256, gs_ft320, gs_ft32bk64, gs_ft64bk64, gs_ft128bk64x6 };

namespace sel {

// the kernels' fixed sizes that the rules lean on (the .hip files assert that theirs are these)
constexpr int kSmallMaxK = 2048;    // fdnn_small.hip: 8 waves x 256 bytes of K
constexpr int kSmallFrameTile = 32;
constexpr int kPpFrameTile = 320;   // fdnn_pp.hip / fdnn_ppo.hip: two 160-frame halves per tile
constexpr int kPpNodeTile = 256;
constexpr int kPpK = 2048;          // 16 ticks of 128 bytes per phase
constexpr int kPpoNodeTiles = 32;   // fdnn_ppo.hip: rows_pad = 8192

// today's defaults
constexpr int kChainMinFrames = 9800;  // chain_ok
constexpr int kChainIdleCus = 24;
constexpr int kPpMinFrames = 16384;    // pp_ok
constexpr int kSmallMaxHidden = 1400, kSmallMaxOutput = 512;  // small_pick
constexpr int kL0SmallMax = 128;  // one round of 32 x 32 tiles on a 2048-node layer; beyond, the (16 | 32) x 64 tiles are as fast
constexpr int kL0SplitMin = 560;  // whole call at 512 / 600 frames: 118 / 140 us with the 64 x 64 tiles, 121 / 136 with the screening

// an int that fdnn_debug_set_* may store while scoring threads read it
struct Switch {
  std::atomic<int> v;
  Switch(int x) : v(x) {}
  Switch(const Switch &o) : v(int(o)) {}
  Switch &operator=(int x) { return v.store(x, std::memory_order_relaxed), *this; }
  Switch &operator=(const Switch &o) { return *this = int(o); }
  operator int() const { return v.load(std::memory_order_relaxed); }
};

// Every switch the rules read.  The process's instance (tuning()) is filled from the environment at first use.
struct Tuning {
  // deployment switches and test hooks: always read
  int chain_env = -1, chain_min_env = kChainMinFrames;       // FDNN_CHAIN, FDNN_CHAIN_MIN
  int pp_env = -1, pp_min_env = kPpMinFrames, pp_only = -1;  // FDNN_PP, FDNN_PP_MIN, FDNN_PP_ONLY (the one hidden layer that may take it)
  int ppo_env = -1;                                          // FDNN_PPO
  int fuse_norm = -1;     // FDNN_FUSE_NORM: 0 never fuse the soft-max, 1 always, -1 not set
  int gemm_debug = 0;     // FDNN_GEMM_DEBUG: test hook, bit 4096 makes fused soft-max tiles give up
  int l0_chain_tn = 64;   // FDNN_L0_TN: test hook, 128 = the round-1 tile shape of the layer-0 chain kernel, kept selectable
  bool chunk_set = false; // FDNN_CHUNK_FRAMES: measurement switch (frame_chunks)
  int chunk_frames = 0;
  // measurement builds only (-DFDNN_ABLATION; FDNN_TUNE_ENV is null otherwise)
  int frame_tile = 0, node_tile = 0, small_max = -1, small_wm = 0, small_ntm = 0, chain_tile = 0;  // FDNN_FRAME_TILE, _NODE_TILE, _SMALL_MAX, _SMALL_WM, _SMALL_NTM, _CHAIN_TILE
  bool small_bk64 = false;  // FDNN_SMALL_BK=64: the three small-launch shapes with 64-byte k-steps in a 6-stage ring
  int fuse_stagger = 0;     // FDNN_FUSE_STAGGER
  bool l0_fma_valu = false, l0_no_screen = false, l0_classic = false, l0_no_split = false;  // FDNN_L0_FMA_VALU, _NO_SCREEN, _CLASSIC, _NO_SPLIT
  int l0_small_max = kL0SmallMax, l0_split_min = kL0SplitMin, l0_t64_bk = 0, l0_screen_wfr = 4, l0s_wn = 0;  // FDNN_L0_SMALL_MAX, _SPLIT_MIN, _T64_BK, _SCREEN_WFR, FDNN_L0S_WN
  int l0_fix_nb = 0, l0_fix_t = 0, l0_fix_lpo = 0;  // FDNN_L0_FIX_NB / _T / _LPO force a fix-list variant
  // run-time overrides (fdnn_debug_set_chain / _pp / _ppo / _fuse): -1 = by the environment
  Switch chain_mode{-1}, chain_min{0}, pp_mode{-1}, pp_min{0}, ppo_mode{-1}, fuse_mode{-1};
};
Tuning &tuning();  // fdnn_select.cpp

struct Device {
  int cus = 256;
};

// "forced mode, else the environment's, else the default; forced minimum, else the environment's"
struct Mode {
  int mode;        // 0: never, 1: wherever the shape allows, -1: by size
  int min_frames;
  bool forced_on;  // the run-time override itself says 1 (tests / measurements)
};
inline Mode resolve_mode(int forced, int forced_min, int env_mode, int env_min) {
  return {forced >= 0 ? forced : env_mode, (forced >= 0 && forced_min > 0) ? forced_min : env_min, forced == 1};
}

// ------------------------------------------------------------------------------------------------------ int8 layers
struct LayerShape {
  int rows, rows_pad, K;  // K = padded input width (bytes per weight row)
  bool fastdiv;           // the 3-operation division was validated for the layer's coefficient
  bool has_fix;           // the layer has saturating pairs
  bool output;
};
struct LayerCall {
  int n;
  int index = 0;           // hidden layers: which one (FDNN_PP_ONLY)
  bool tap_acc = false, tap_logit = false, acc_probe = false;
  bool byte_mask = false, bit_mask = false;  // lazy contract: the caller's mask
  bool may_fuse = true;    // output layer: context, process and model allow the fused soft-max
};
enum class Form { small, tiled, pp, ppo };
struct LayerChoice {
  Form form;
  int frame_tile, node_tile, n_pad;
  GemmShape shape;  // tiled
  int small_ntm;    // small, hidden: 1 = 32-node tiles, 2 = 64-node tiles
  bool fused;       // output: soft-max scaled inside the kernel
  int partial_ld;   // output: row length of the soft-max partial sums (the in-phase tiling's n_pad, role-split or not)
  bool mask_bits;   // output: the masked instances read the mask as bits (else: as bytes)
};

inline int round_up_to(int n, int t) { return (n + t - 1) / t * t; }

// Frame tile (32/64/128/256/320) of the tiled int8 GEMM for `n` frames of a layer with rows_pad padded nodes;
// *from_model: the cost model chose (not the one-round loop).
inline int frame_tile(int rows_pad, int n, const Tuning &t, bool *from_model = nullptr) {
  if (from_model) *from_model = false;
  const int forced = t.frame_tile;
  if (forced == 32 || forced == 64 || forced == 128 || forced == 256 || forced == 320) return forced;
  const int mt = rows_pad / 256;
  // Few frames: while every workgroup gets a CU of its own the launch is one k-loop deep and
  // latency bound, so the smallest tile that still fits in one round wins -- it has the shortest
  // k-step and puts the most CUs to work (2048 x 2048 layer, 1000 frames: 21 us with 32-frame
  // tiles = 256 workgroups, 24 us at 64, 31 us at 128; 8000-node output layer, 1000 frames:
  // 39 us at 128 = 256 workgroups, 47 us at 64, 65 us at 32 = four rounds).
  for (int ft : {32, 64, 128})
    if (static_cast<long>(mt) * ((n + ft - 1) / ft) <= 256) return ft;
  // Cost model: rounds x frames per tile / relative throughput of the kernel shape.
  // A round fills every CU once (two co-resident workgroups for the 4-wave shapes).
  struct Cand {
    int ft, slots;
    double eff;
  };
  const Cand cands[] = {{128, 512, 0.55}, {256, 256, 1.0}, {320, 256, 1.0}};
  int best = 128;
  double best_cost = -1.0;
  for (const Cand &c : cands) {
    const long blocks = static_cast<long>(mt) * ((n + c.ft - 1) / c.ft);
    const long rounds = (blocks + c.slots - 1) / c.slots;
    // a 4-wave workgroup shares its CU with a second one: a round costs two tiles' time
    const double cost = rounds * c.ft * (c.slots == 512 ? 2.0 : 1.0) / c.eff;
    if (best_cost < 0 || cost < best_cost || (cost == best_cost && c.ft > best)) {
      best_cost = cost;
      best = c.ft;
    }
  }
  if (from_model) *from_model = true;
  return best;
}

// Small-batch shape (fdnn_small.hip) available for this layer?  (K up to 8 slices of 256 bytes; the exact-division /
// bounded-range epilogue only; taps of the output layer need a mask-capable instance, which the tap instance is.)
inline bool small_ok(int K, bool fastdiv) { return fastdiv && K <= kSmallMaxK; }

// Batches up to this many frames take the small-batch kernel where the layer allows it.  Measured
// crossovers on the 2048-wide layers (tools/batch_sweep.py, FDNN_SMALL_MAX=0 against the default): six hidden layers
// (64-node tiles from ~160 frames up) 54 vs 88 us at 256 frames, 68 vs 90 at 512, 93 vs 104 at 1000, 104 vs 118 at
// 1200, 117 vs 118 at 1500, 137 vs 121 at 2000; the 8000-node output layer 16.5 vs 24.6 at 256, 25.8 vs 26.3 at 512,
// 44 + 15 (scale pass) vs 40 (fused) at 1000 (a workgroup of the small kernel walks its frame tiles one after the other).
inline bool small_pick(const LayerShape &l, int n, const Tuning &t) {
  const int lim = t.small_max >= 0 ? t.small_max : l.output ? kSmallMaxOutput : kSmallMaxHidden;
  return n <= lim && small_ok(l.K, l.fastdiv);
}

// Mid-size batches of the hidden layers: when the layer is between one and two rounds of 128 x 128 tiles (2 049 .. 4 096
// frames on a 2048-node layer), the four-wave 128 x 128 shape -- two workgroups per CU, so one's prologue / epilogue
// hides under the other's k-loop -- beats the 256-node tiles of the same area (tools/batch_sweep.py, six hidden layers:
// 140 vs 158 us at 2 560 frames, 141 vs 158 at 3 000, 151 vs 162 at 4 000; it loses below (123 vs 119 at 2 000: one
// workgroup per CU again) and above (229 vs 202 at 5 000), and on the 8000-node output layer).  Returns 128 or 256;
// with 128 the frame tile is 128 as well.
inline int node_tile(int rows_pad, int n, bool output, const Tuning &t) {
  if (output) return 256;
  if (t.node_tile == 128 || t.node_tile == 256) return t.node_tile;
  const long tiles = static_cast<long>(rows_pad / 128) * ((n + 127) / 128);
  return (tiles > 256 && tiles <= 512) ? 128 : 256;
}

// a 128-frame launch of at most 256 workgroups, every one with a CU of its own (no taps): the one latency-bound k-loop per
// launch takes whole cache lines per step (128-byte k-steps); every other 128-frame launch the 64-byte-step shape
inline bool ft128_one_round(int rows_pad, int n_pad, bool tap_acc) { return static_cast<long>(rows_pad / 256) * (n_pad / 128) <= 256 && !tap_acc; }

// The tile shape of a tiled launch.
// Few frames: 32- / 64-frame tiles put four / two times as many workgroups on the chip; 128-byte
// k-steps (3-stage ring) halve the barriers of the latency-bound loop: 16.6 vs 21 us per
// 2048 x 2048 layer.  What is left at this size is mostly the launch itself: a 128-node tile
// (half the operand traffic per workgroup) and whole-step fragment prefetch, both tried, left
// the 16.6 us untouched.
// ... and while the 32-frame tiles leave CUs idle or nearly so, a launch waits for ONE workgroup's operand stream: 288
// rows x 2 KiB at the ~70 GB/s one CU's LDS-DMA path moves = 8 of the 17 us of a 2048 x 2048 layer, whatever the frame
// count.  64-node tiles (one wave per workgroup) split the same weight rows over four times as many CUs: six hidden
// layers 101-110 -> 88-98 us from 8 to 700 frames (tools/batch_sweep.py; up to three workgroups per CU, beyond that
// the extra activation traffic loses).  Hidden layers only: the output layer's exp / transposition epilogue makes its
// narrow tiles slower (27 vs 21 us).
inline GemmShape gemm_shape(const LayerShape &l, int ft, int nt, int n_pad, bool tap_acc, const Tuning &t) {
  if (!l.fastdiv) return gs_tdiv;  // layer whose coefficient failed the exact-division check (e.g. 127/0 = inf)
  switch (ft) {
    case 32: {
      if (t.small_bk64) return gs_ft32bk64;
      bool one_wave = !l.output && static_cast<long>(l.rows_pad / 256) * (n_pad / 32) * 4 <= 768;
      if (!l.output && t.small_wm) one_wave = t.small_wm == 1;  // FDNN_SMALL_WM=1 / 4: one wave per workgroup or four, whatever the launch's size
      return one_wave ? gs_ft32w1 : gs_ft32;
    }
    case 64: return t.small_bk64 ? gs_ft64bk64 : gs_ft64;
    case 128:
      if (!l.output && nt == 128) return gs_ft128nt128;  // 128 nodes x 128 frames, 2 x 2 waves, double-buffered 128-byte k-steps, two workgroups per CU
      if (!ft128_one_round(l.rows_pad, n_pad, tap_acc)) return gs_ft128;  // 4 waves, 3-stage ring, two workgroups per CU
      return t.small_bk64 ? gs_ft128bk64x6 : gs_ft128bk128;
    case 256: return gs_ft256;  // 8 waves, 128-byte k-step (whole cache lines), double buffer, one workgroup per CU
    default: return gs_ft320;
  }
}

// Fused soft-max available for this launch?  (dense production call or bit masks, 8-wave shapes and the one-round 128-frame
// shape, the row sums of all node tiles fit the epilogue's LDS)
inline bool fused_ok(const LayerShape &l, const LayerCall &c, const LayerChoice &ch, const Tuning &t) {
  const bool mask = c.byte_mask || c.bit_mask;
  if (t.fuse_norm == 0 || ch.form == Form::small || ch.node_tile != 256 || !l.fastdiv || (mask && !ch.mask_bits) || c.tap_acc || c.tap_logit) return false;
  if (ch.frame_tile != 320 && ch.frame_tile != 256 && ch.frame_tile != 128) return false;
  // the 128-frame tiles of more than one round have no fused form: none can come about here, where MT <= 32 below and
  // frame_tile's cost model prefers 128 from 129 node tiles up (a forced FDNN_FRAME_TILE apart)
  if (ch.frame_tile == 128 && !ft128_one_round(l.rows_pad, ch.n_pad, c.tap_acc)) return false;
  const int MT = l.rows_pad / 256;
  int L = 1;
  while (L < MT) L <<= 1;
  // the epilogue's LDS: one 32 x 64 float tile per wave, then 4 partial rows + the inverses + L rows of S, below the
  // table / bias area (GemmCfg::FIX_OFF: two 128-byte-step stages for the 8-wave shapes, at least three 64-byte-step
  // stages for the 4-wave ones)
  const bool eight = ch.frame_tile >= 256;
  const long need = 8192 + (eight ? 8 : 4) * 32 * 68 * 4 + (5L * ch.frame_tile + 4 + static_cast<long>(L) * ch.frame_tile) * 4;
  const long have = static_cast<long>(256 + ch.frame_tile) * (eight ? 128 * 2 : 64 * 3);
  return L <= 32 && need <= have;
}

// The role-split kernel (fdnn_pp.hip) serves the production shape (K = 2048: 16 ticks per phase, 256-node tiles, validated
// 3-operation division).  Where it pays today (profiles/LABBOOK.md, round 6): layers WITHOUT saturating pairs from two tiles per
// workgroup up (16 384 frames on a 2048-wide net: 463 vs 480 us for six layers at 20 000 frames; 260 vs 258 at 10 000, where a
// workgroup has one tile and nothing hides the second half's epilogue).  With the pair-saturation walk in the compute
// role's instruction stream -- one wave per SIMD, nothing to cover its latency chain -- it loses (328 vs 279 us on the
// Gaussian bench net): such layers keep fdnn_gemm.hip's in-phase tiles unless forced (fdnn_debug_set_pp(1, n), FDNN_PP=1).
inline bool pp_ok(const LayerShape &l, int n, const Tuning &t) {
  const Mode m = resolve_mode(t.pp_mode, t.pp_min, t.pp_env, t.pp_min_env);
  if (m.mode == 0 || !l.fastdiv || l.K != kPpK || l.rows_pad % kPpNodeTile != 0) return false;
  if (m.mode != 1 && l.has_fix) return false;
  return n >= m.min_frames;
}

// The role-split fused output kernel (fdnn_ppo.hip) serves the dense production call of the 8000-node layer (8192 padded
// rows = 32 node tiles: the row sums of a half are one 20 KB block; K = 2048; validated 3-operation division; rows % 4 == 0)
// on a device whose CUs can hold one workgroup per (node tile, frame pair slot): grid = 32 x (CUs / 32).
inline bool ppo_ok(const LayerShape &l, int n, const Tuning &t) {
  const Mode m = resolve_mode(t.ppo_mode, 0, t.ppo_env, 0);
  if (m.mode == 0 || !l.fastdiv || l.K != kPpK || l.rows_pad != kPpoNodeTiles * kPpNodeTile || (l.rows & 3) != 0) return false;
  if (m.mode == 1) return true;
  // By default where it was measured ahead of the in-phase fused tiles (tools/ppo_time.py, several boxes; LABBOOK round 6).
  // A launch is ceil(pairs / 8) rounds of frame pairs (8 slots of 32 workgroups on 256 CUs); what matters is how full the
  // last round is and that a workgroup has at least two pairs (a steady state):
  //   a layer without saturating pairs (trained nets): from 14 pairs when the rounds are >= 3/4 full -- 4 480 frames 102 us
  //   against 105, 5 120: 105 / 113, 10 000: 191 .. 212 / 218 .. 226, 20 480: 391 / 444; 3 840 (12 pairs): 100 / 95;
  //   a layer with pairs (the walk runs in a lone compute wave): from 22 pairs when the rounds are >= 4/5 full -- 7 000 frames
  //   170 / 173, 7 680: 171 / 178, 8 320 .. 8 960: 217 / 224 .. 226, 10 000: 223 / 232, 12 000: 272 / 298, 16 000: 382 / 407;
  //   8 000 (25 pairs: four rounds, the last with one pair): 216 / 200; 5 120: 123 / 117.
  const int pairs = (n + kPpFrameTile - 1) / kPpFrameTile, rounds = (pairs + 7) / 8;
  return l.has_fix ? pairs >= 22 && 5 * pairs >= 4 * 8 * rounds : pairs >= 14 && 4 * pairs >= 3 * 8 * rounds;
}

// One int8 layer over the call's frames: the form, its tiles and, for the output layer, whether the soft-max is fused.
inline LayerChoice choose_layer(const LayerShape &l, const LayerCall &c, const Tuning &t) {
  LayerChoice ch{};
  const bool small = small_pick(l, c.n, t);
  ch.form = small ? Form::small : Form::tiled;
  ch.frame_tile = small ? kSmallFrameTile : l.fastdiv ? frame_tile(l.rows_pad, c.n, t) : 128;  // the true-divide kernel has one shape
  ch.node_tile = (!small && l.fastdiv) ? node_tile(l.rows_pad, c.n, l.output, t) : 256;
  if (ch.node_tile == 128) ch.frame_tile = 128;
  ch.n_pad = ch.partial_ld = round_up_to(c.n, ch.frame_tile);
  // Hidden layers, small: 32-node tiles while a frame tile per workgroup fills the chip (up to ~128 frames on a 2048-node
  // layer); beyond, 64-node tiles halve the activation bytes per output (each workgroup then walks fewer frame tiles).
  // FDNN_SMALL_NTM=1|2 forces one shape (measurements).  The output layer has the 64-node tiles only.
  const long wg32 = static_cast<long>(l.rows_pad / 32) * (ch.n_pad / kSmallFrameTile);
  ch.small_ntm = l.output ? 2 : t.small_ntm ? (t.small_ntm == 2 ? 2 : 1) : wg32 > 320 ? 2 : 1;
  if (!l.output) {
    // Large batches of the production shape: the role-split kernel -- one wave of each SIMD in the k-loop, its partner
    // staging that tile's operands and running the epilogue of the tile before.  Identical bytes.
    if (!c.tap_acc && pp_ok(l, c.n, t) && (t.pp_only < 0 || t.pp_only == c.index)) {
      ch.form = Form::pp;
      ch.frame_tile = kPpFrameTile;
      ch.n_pad = round_up_to(c.n, ch.frame_tile);
    }
  } else {
    // large-batch production instances: the mask travels as bits (one 64-bit word per frame row and 64-node group); the
    // small-batch and the tap instances read bytes
    ch.mask_bits = (c.byte_mask || c.bit_mask) && !small && !c.tap_acc;
    ch.fused = c.may_fuse && fused_ok(l, c, ch, t);  // (taps exclude it; the accumulator probe of the parity tests does not)
    // the role-split fused kernel: dense, unprobed, the production shape, enough frames for a steady state
    if (ch.fused && !c.byte_mask && !c.bit_mask && !c.acc_probe && ppo_ok(l, c.n, t)) {
      ch.form = Form::ppo;
      ch.frame_tile = kPpFrameTile;
      ch.n_pad = round_up_to(c.n, ch.frame_tile);
    }
  }
  ch.shape = gemm_shape(l, ch.frame_tile, ch.node_tile, ch.n_pad, c.tap_acc, t);
  return ch;
}

// ------------------------------------------------------------------------------------- the hidden layers of a pass
// From ~9 800 frames up -- a round of 256-node x 320-frame tiles and more -- the chain is the faster form at EVERY size
// (tools/chain_sweep.py, layer 0 + six hidden layers, chained / per-layer: 10 000 frames 0.98, 10 241 0.88, 12 000 0.86,
// 15 360 0.93, 20 480 0.97): its tasks flow across the layers where a launch per layer idles most of the chip in every
// partial round.  Below, the per-layer path has better tiles for the size (160- / 128-frame four-wave shapes, two workgroups
// per CU) and the chain's 320-frame tasks leave CUs without work: 9 000 frames 1.04, 8 000 1.21, 6 000 1.33, 4 097 1.33.
inline bool chain_ok(int rows_pad, int K, int n, int n_layers, const Tuning &t, const Device &dev) {
  const Mode m = resolve_mode(t.chain_mode, t.chain_min, t.chain_env, t.chain_min_env);  // 0: never; otherwise from min_frames up
  if (m.mode == 0 || n_layers < 2 || n_layers > kMaxChainLayers || K % 128 != 0 || n < m.min_frames) return false;
  if (m.forced_on) return true;  // (tests / measurements: wherever the shape allows)
  // ... and only where a launch per layer would run a partly filled round: at whole rounds of 320-frame tiles (10 000 /
  // 10 240 / 20 480 frames on a 2048-wide net) the two forms are within +-2 % of each other, the sign depending on the box.
  const long cus = dev.cus;
  const long tiles = static_cast<long>(rows_pad / 256) * ((n + 319) / 320);
  const long idle = (tiles + cus - 1) / cus * cus - tiles;
  return idle >= kChainIdleCus;
}

// Frame tile of the chained launch: 320-frame tiles unless the padding they add is worth more than their better operand reuse
inline int chain_frame_tile(int n, const Tuning &t) {
  if (t.chain_tile == 256 || t.chain_tile == 320) return t.chain_tile;
  const int pad320 = (n + 319) / 320 * 320 - n, pad256 = (n + 255) / 256 * 256 - n;
  return pad256 + 64 < pad320 ? 256 : 320;
}

struct HiddenPlan {
  bool chain;             // the int8 hidden layers as persistent launches of up to kMaxChainLayers layers each (else: a launch per layer)
  int frame_tile, n_pad;  // chained
};
// layers of the chained launch that starts at hidden layer q0 (nets deeper than kMaxChainLayers + 1: several chains)
inline int chain_segment(int n_hid, int q0) { return std::min(kMaxChainLayers, n_hid - q0); }

// `layer(i)` -> LayerShape of int8 hidden layer i.  All hidden layers of a net have the same shape (README.md:10), so one
// set of sizes serves every layer of a chain: a net whose layers differ, or with a layer without the validated division,
// does not chain.  `allowed`: what the rules cannot see -- no taps, a context with healthy chain counters.
template <class LayerAt>
HiddenPlan plan_hidden(int n_hid, LayerAt layer, int n, bool allowed, const Tuning &t, const Device &dev) {
  HiddenPlan p{false, 0, 0};
  if (!allowed || n_hid < 2) return p;
  const LayerShape l0 = layer(0);
  if (!chain_ok(l0.rows_pad, l0.K, n, std::min(n_hid, kMaxChainLayers), t, dev)) return p;
  for (int i = 0; i < n_hid; ++i) {
    const LayerShape l = layer(i);
    if (!(l.fastdiv && l.rows == l0.rows && l.rows_pad == l0.rows_pad && l.K == l0.K)) return p;
  }
  p.chain = true;
  p.frame_tile = chain_frame_tile(n, t);
  p.n_pad = round_up_to(n, p.frame_tile);
  return p;
}

// ----------------------------------------------------------------------------------------------------------- layer 0
// LDS the small-batch kernel needs for input width D (0: does not fit, or the division magics are not exact)
inline unsigned l0_div_magic(int d, int max_c) {
  const unsigned m = static_cast<unsigned>((0x100000000ull + static_cast<unsigned>(d) - 1) / static_cast<unsigned>(d));
  for (int c = 0; c <= max_c; ++c)
    if (static_cast<int>((static_cast<unsigned long long>(c) * m) >> 32) != c / d) return 0;
  return m;
}
struct L0SmallGeom {
  int sc = 0, lds = 0;
  unsigned sc_magic = 0, ch_magic = 0;
};
inline L0SmallGeom l0_small_geom(int D) {
  L0SmallGeom g;
  const int ch = D / 4, sc = ch | 1;
  const int n_ld = (32 * sc + 63) / 64;
  const int bytes = 2 * n_ld * 1024 + 2 * ((D * 4 + 1023) & ~1023) + 2048 + 64;
  if (ch < 2 || bytes > 160 * 1024) return g;  // (ch = 1: the magic 2^32 does not fit 32 bits)
  g.sc_magic = l0_div_magic(sc, n_ld * 64 + 64);
  g.ch_magic = l0_div_magic(ch, 32 * ch + 512);
  if (!g.sc_magic || !g.ch_magic) return g;
  g.sc = sc;
  g.lds = bytes;
  return g;
}
// int8 screening (fdnn_l0s.hip) available for this layer shape?
// D <= 496: 256 P0 + P1 stays inside int32 (2^22 D + 2^15 D < 2^31) and the pre-pass rows fit its LDS
inline bool l0_split_ok(int D, int H) { return D >= 64 && D <= 496 && (D & 3) == 0 && (H & 15) == 0; }

struct L0Call {
  int D, H, h_ld, n, n_rows;
  bool fma;     // flavour: 0 mul then add (canonical), 1 fused
  int kernel;   // requested kind (L0Params::kernel): 0 pick by batch size, 1 chain, 2 64 x 64 tiles, 3 screened, 4 split
  bool taps;
  bool chain_images;  // which scratch exists: the chain-major operand images,
  bool screen_lists;  // the node norms and per-tile lists of the screened path,
  bool split_planes;  // the digit planes, constants, table and list of the int8 screening (and the per-tile lists)
};
enum class L0Kind { mfma, small, split, screened, chain, tile64 };
struct L0Choice {
  L0Kind kind;
  int tile;       // tile64: 16 / 32 / 64 frames per tile; screened: 4 = 128 x 128 tiles, 2 = 64 x 128; chain: the node tile (64 / 128)
  int split_wn;   // split: 1 = 64-node tiles, 2 = 128-node tiles
  int fix_nb, fix_threads, fix_lpo;  // split: the fix-list variant {blocks in flight, threads, lanes per output}
};

inline L0Choice choose_l0(const L0Call &p, const Tuning &t) {
  L0Choice ch{};
  if (p.fma && !t.l0_fma_valu) {
    // 32-float chunks, 4 x 2 waves (128 x 128 tile).  Measured alternatives at 10 000 frames:
    // 16-float chunks 0.221 ms, 64-float 0.205, 256-thread workgroups (two per CU) 0.205.
    ch.kind = L0Kind::mfma;
    return ch;
  }
  // Small batches (canonical flavour): the whole-K kernel, 32 x 32 tiles (100 frames: 20 -> 6 us)
  if (!p.fma && p.kernel == 0 && p.n_rows <= t.l0_small_max && l0_small_geom(p.D).lds > 0) {
    ch.kind = L0Kind::small;
    return ch;
  }
  // Three bit-identical candidates, chosen by modelled time (432 -> 2048 layer, tools/l0_kind_sweep.py; all three
  // come in rounds of 256 tiles, one per CU, and a round costs the same full or not):
  //   screened   fused chains on the matrix pipe + exact recomputation of the few outputs the fusion could change
  //              (128 x 128 tiles): 74 / 122 / 174 / 234 / 285 us for 1..5 rounds; large batches without taps only
  //   chain      all-VALU chain kernel (128 frames x 64 nodes): 57 / 82 / 110 / 142 / 171 / 203 us for 1..6 rounds
  //   tile64     (16 | 32 | 64) x 64 tiles, 4 outputs x 4 chains per thread and frame: 19-23 us up to 400 frames, 33-49 us up to
  //              1200, then 20 us + 35.5 ns per frame
  // e.g. 2560 frames: 120 screened, 109 chain; 3000: 110 chain, 125 the others; 6000: 174 screened, 204 chain.
  const double work = static_cast<double>(p.D) / 432.0;
  const long ft128 = (p.n_rows + 127) / 128;
  const double screened_us = 18.0 + 54.0 * work * static_cast<double>((ft128 * ((p.H + 127) / 128) + 255) / 256);
  const double chain_us = 27.0 + 30.0 * work * static_cast<double>((ft128 * (p.h_ld / t.l0_chain_tn) + 255) / 256);
  const double tile64_us = p.n_rows <= 320    ? 23.0 * work
                           : p.n_rows <= 1200 ? (17.0 + 0.032 * p.n_rows) * work
                                              : 20.0 + 0.0355 * work * (p.H / 2048.0) * p.n_rows;
  const bool can_screen = !p.fma && !t.l0_no_screen && (p.kernel == 0 || p.kernel == 3) && !p.taps && p.screen_lists && p.n >= 2048 &&
                          p.D <= 4096;  // l0_fix_kernel: 8 D bytes of shift / scale + 24 KB of product blocks in dynamic LDS (64 KB without an attribute)
  const bool can_chain = !p.fma && p.chain_images && p.kernel != 2 && !(t.l0_classic && p.kernel == 0);
  // Round 4: the screening on the int8 matrix pipe (fdnn_l0s.hip: exact 24-bit integer images of both operands, eight
  // int8 MFMA products) + the same exact recomputation of the flagged outputs.  128 x 128 tiles, 1.85 us of matrix-pipe
  // time per tile and CU at peak: from FDNN_L0_SPLIT_MIN frames up it replaces all of the above.
  const bool can_split = !p.fma && !t.l0_no_split && !t.l0_no_screen && (p.kernel == 0 || p.kernel == 4) && !p.taps && p.split_planes && l0_split_ok(p.D, p.H);
  if (can_split && (p.kernel == 4 || p.n >= t.l0_split_min)) {
    ch.kind = L0Kind::split;
    // 128-node tiles, one 512-thread workgroup per CU; batches so small that those would leave half the chip idle (up to 128
    // tiles: 1 024 frames on a 2048-node layer) take 64-node tiles, twice as many workgroups of half the size.  Measured
    // equal both where both fill the chip (99.2 vs 97.7 us at 10 000 frames) and below (layer 0 at 1 000 frames 40.2 vs 40.4 us:
    // one tile's latency -- 16 chunks and a 32-output-per-lane epilogue per wave -- either way).  FDNN_L0S_WN=1|2 forces one.
    const int tiles128 = ((p.n_rows + 127) / 128) * (p.h_ld / 128);
    ch.split_wn = t.l0s_wn == 1 || t.l0s_wn == 2 ? t.l0s_wn : (tiles128 <= 128 ? 1 : 2);
    // Fix-list variant by batch size (rocprofv3, us at 1 000 / 4 000 / 10 000 frames; LABBOOK): four lanes per output, three quads per
    // lane and operand in flight, 256 threads: 8.7 / 11.4 / 23.8; EIGHT lanes per output (a whole 128-byte line per output
    // and load, five round trips instead of nine): 7.3 / 13.8 / 25.0 -- fewer flagged outputs = a latency chain, many = L2
    // gathers, where the second set of lanes only costs registers.  FDNN_L0_FIX_NB / _T / _LPO force a variant.
    ch.fix_threads = t.l0_fix_t == 512 ? 512 : 256;
    ch.fix_lpo = t.l0_fix_lpo ? (t.l0_fix_lpo == 8 ? 8 : 4) : (p.n_rows < 3000 ? 8 : 4);
    const int nb = t.l0_fix_nb ? t.l0_fix_nb : 3;
    ch.fix_nb = ch.fix_lpo == 8 ? (nb >= 3 ? 3 : 2) : (nb >= 5 ? 5 : 3);
    return ch;
  }
  if (can_screen && (p.kernel == 3 || (screened_us < (can_chain ? chain_us : tile64_us) && screened_us < tile64_us))) {
    // 4: 128 x 128 tiles, one 512-thread workgroup per CU; 2: 64 x 128 tiles, two 256-thread workgroups per CU
    // (one's screening epilogue under the other's matrix stream, and half the batch-size staircase)
    ch.kind = L0Kind::screened;
    ch.tile = t.l0_screen_wfr == 2 ? 2 : 4;
    return ch;
  }
  if (can_chain && (p.kernel == 1 || chain_us < tile64_us)) {
    // Node tile of the chain kernel: 64 (8 frames x 4 nodes per thread, every partial sum in registers,
    // three workgroups per CU) or 128 (8 x 8, l2 + l3 parked in a global scratch buffer).  Both run
    // at the same speed -- the kernel is bound by vector-instruction issue, 329.8 vs 331.7 us at
    // 10 000 frames (rocprofv3) -- but the 64-wide tile moves 164 MB less through HBM per launch and
    // needs no scratch, which is what the soft-max scale running underneath it in the server loop
    // competes for.  FDNN_L0_TN=128 selects the round-1 shape.
    ch.kind = L0Kind::chain;
    ch.tile = t.l0_chain_tn;
    return ch;
  }
  // 64 x 64 tile, 16-float chunks, 4 x 4 outputs per thread.  Measured alternatives: 32-float
  // chunks 0.448 ms, 8 x 4 outputs per thread 0.468 / 0.477 ms (occupancy 2) against 0.388.
  // Few frames: a 64 x 64 tile is 30-40 us of dependent vector work for ONE workgroup however few of them there are, so
  // small batches take 16- / 32-frame tiles (more, shorter workgroups).  Measured (tools/l0_kind_sweep.py), 8 / 100 / 256 /
  // 512 / 1000 frames: 16 x 64 tiles 19 / 21 / 23 / 38 / 60 us, 32 x 64 27 / 30 / 30 / 33 / 49, 64 x 64 43 / 45 / 45 / 45 / 55.
  ch.kind = L0Kind::tile64;
  ch.tile = (t.l0_t64_bk == 164 || (t.l0_t64_bk == 0 && p.n_rows <= 320)) ? 16 : (t.l0_t64_bk == 232 || (t.l0_t64_bk == 0 && p.n_rows <= 1200)) ? 32 : 64;
  return ch;
}

}  // namespace sel
}  // namespace fdnn
