// fdnn_ctx_layout.hpp -- how large a context's scratch buffers are (ctx_layout: what make_ctx allocates, as one pure
// function of the net's shape and the frame count) and what a launch indexes in each of them (the extent functions, from
// the choices of fdnn_select.hpp).  No HIP in here: tests/host/ctx_layout_check.cpp asserts on the host that every extent
// of every launch the selection can choose stays inside the layout -- a shortfall would be a write past a scratch buffer.
#pragma once
#include <algorithm>
#include <cstddef>

#include "fdnn_model.hpp"  // kColPad, kRowSkew
#include "fdnn_select.hpp"

namespace fdnn {

constexpr int kMaxFrameTile = 320;  // largest GEMM frame tile; scratch rows carry this much slack
constexpr int kPartialNodes = 64;   // nodes covered by one soft-max partial sum
constexpr int kL0ScreenCap = 4096;  // layer 0, screened: listed outputs per tile (25 %); a tile that overflows is recomputed whole
constexpr int kPinFrames = 8;       // per-frame lazy calls: frames of host-mapped staging (fdnn_ctx::h_mask_pin, h_out_pin)
constexpr int kChainCtlWords = 16;  // chained launch: queue heads [0..7], workgroups that left [8]

// int8 screening (fdnn_l0s.hip): chains padded to whole chunk pairs (432 -> 4 x 128 positions, 16 chunks); bytes of one operand's digit planes
inline int l0_split_chain_pad(int D) { return (D / 4 + 63) / 64 * 64; }
inline int l0_split_chunks(int D) { return 4 * l0_split_chain_pad(D) / 32; }
inline size_t l0_split_plane_bytes(int D, int rows_ld) { return static_cast<size_t>(l0_split_chunks(D)) * 3 * static_cast<size_t>(rows_ld / 32) * 1024; }

struct CtxShape {  // what the sizes depend on, and nothing else
  int in_dim, hidden, out_dim, max_rows_pad;  // max_rows_pad: the largest rows_pad of the int8 layers
  int l0_j_pad, l0_h_ld;         // the model's layer-0 image: chain rows, node row length
  bool split;                    // the model has the int8-screening planes (sel::l0_split_ok)
  int l0_chain_tn, l0_list_cap;  // sel::Tuning::l0_chain_tn: 128 parks partial sums; > 0: caps the flagged-output list (tests)
  bool lean;                     // a scoring-loop slot: no frame / result / mask buffers, no pinned staging
  int n;
};
// Element counts of everything make_ctx allocates, in its order; 0 = not allocated for this shape.
struct CtxLayout {
  int cap, act_ld, xt_ld, glist_cap;
  size_t x, xt;                // float [cap][D], [4][l0_j_pad][xt_ld]
  size_t scr_count, scr_list;  // uint32 [tiles], uint16 [tiles][kL0ScreenCap]
  size_t xd, xstat;            // int8 digit planes, float [3][xt_ld]
  size_t glist_count, l0park;  // uint32 [2] beside uint2 [glist_cap]; float [xt_ld][l0_h_ld]
  size_t act, out;             // int8 [cap + kMaxFrameTile][act_ld] each of the two, float [cap][O]
  size_t partial, mask, mask_bits;  // float [max_rows_pad / kPartialNodes][cap + kMaxFrameTile], int8 [cap][O], uint64 [cap][ceil(O / 64)]
  size_t fuse_s, fuse_cnt, fuse_flag, chain_ctl, chain_done;
  size_t mask_pin, out_pin;    // host-mapped: int8, float
};

// The self-rewinding scratch: counter arrays that make_ctx zeroes once, that every launch assumes zero
// on entry and that only the kernels themselves put back to zero before they end.  One row per buffer, 32-bit words each;
// the scratch audit (fdnn_debug_ctx_scratch, fdnn_runtime.cpp: ctx_scratch_buf) counts non-zero words row by row.
// kCtxScratchExempt: counter fields of the layout that are NOT self-rewinding, with who zeroes them before their next reader.
struct CtxScratchRow {
  const char *name;
  size_t CtxLayout::*words;
};
constexpr int kCtxScratchCount = 5;
enum CtxScratchId { kScrCount, kFuseCnt, kFuseFlag, kChainCtl, kChainDone };
inline constexpr CtxScratchRow kCtxScratch[kCtxScratchCount] = {
    {"scr_count", &CtxLayout::scr_count},    // written fdnn_l0.hip (screened) / fdnn_l0s.hip (whole-tile path); rewound by l0_fix_kernel, l0_fix_list_kernel
    {"fuse_cnt", &CtxLayout::fuse_cnt},      // fdnn_gemm.hip: the frame tile's last leaver; fdnn_ppo.hip: the half's last gatherer
    {"fuse_flag", &CtxLayout::fuse_flag},    // fdnn_gemm.hip: lowered by the frame tile's last workgroup
    {"chain_ctl", &CtxLayout::chain_ctl},    // fdnn_chain.hip: the last workgroup out
    {"chain_done", &CtxLayout::chain_done},  // fdnn_chain.hip: the last workgroup out
};
struct CtxScratchExempt {
  const char *name;
  size_t CtxLayout::*words;
  const char *zeroed_by;
};
inline constexpr CtxScratchExempt kCtxScratchExempt[] = {
    {"glist_count", &CtxLayout::glist_count, "the next launch's pre-pass (fdnn_l0s.hip: l0_digits_kernel), in stream order before the screening kernel"},
};

inline CtxLayout ctx_layout(const CtxShape &s) {
  CtxLayout l{};
  l.cap = sel::round_up_to(std::max(s.n, 1), 64);
  l.act_ld = sel::round_up_to(s.hidden, kColPad) + kRowSkew;
  const size_t np = size_t(l.cap);
  // the GEMMs work on whole frame tiles: every frame-indexed scratch carries one
  // tile of slack rows (a launch covers [first, first + round_up(count, tile)))
  const size_t npt = np + kMaxFrameTile;
  if (!s.lean) l.x = np * s.in_dim;
  l.xt_ld = sel::round_up_to(l.cap, 128);
  l.xt = 4 * size_t(s.l0_j_pad) * l.xt_ld;
  // screened layer-0 path: the per-tile lists of outputs to recompute exactly; 64- or 128-frame x 128-node screening tiles
  l.scr_count = size_t(l.xt_ld / 64) * size_t((s.hidden + 127) / 128);
  l.scr_list = l.scr_count * kL0ScreenCap;
  if (s.split) {  // int8 screening: the frames' digit planes and row constants
    l.xd = l0_split_plane_bytes(s.in_dim, l.xt_ld);
    l.xstat = 3 * size_t(l.xt_ld);
    l.glist_cap = int(std::min<size_t>(size_t(l.xt_ld) * size_t(s.l0_h_ld) / 16, size_t(1) << 26));  // 6 % of the outputs
    if (s.l0_list_cap > 0) l.glist_cap = std::min(l.glist_cap, s.l0_list_cap);  // (tests: fdnn_debug_set_l0_list_cap)
    l.glist_count = 2;
  }
  if (s.l0_chain_tn == 128) l.l0park = size_t(l.xt_ld) * s.l0_h_ld;  // (the 64-node tile keeps its partial sums in registers)
  l.act = npt * l.act_ld;
  if (!s.lean) l.out = l.mask = np * s.out_dim;
  l.partial = npt * (s.max_rows_pad / kPartialNodes);
  l.mask_bits = np * size_t((s.out_dim + 63) / 64);
  // fused soft-max (large dense batches): row sums per 256-node tile, counters and flags per frame tile of 128 frames and up
  const size_t mt = size_t(s.max_rows_pad / 256), fuse_tiles = npt / 128 + 2;
  l.fuse_s = npt * mt;
  l.fuse_cnt = 8 * fuse_tiles;
  l.fuse_flag = fuse_tiles * mt;
  // chained hidden layers: queue heads + leave counter, per frame tile and layer the finished node tiles (zero between launches)
  l.chain_ctl = kChainCtlWords;
  l.chain_done = (npt / 256 + 2) * kMaxChainLayers;
  if (!s.lean) l.mask_pin = std::max(size_t(kPinFrames) * s.out_dim, size_t(s.max_rows_pad));  // (at least one padded row of slack)
  if (!s.lean) l.out_pin = size_t(kPinFrames) * s.out_dim;
  return l;
}

// ------------------------------------------------------------------------------------------- what a launch indexes
// Each function says how many elements of a context buffer one launch may touch, from the choice the selection made
// for it; the comment names the kernel lines the figure is read from.  ctx_layout_check.cpp holds extent <= layout count.
constexpr int kL0TileFrames = 128;    // layer 0: frame tile of the chain, int8-screening and 128 x 128 screened kernels
constexpr int kL0TileNodes = 128;     // ... node tile of the per-tile counters (fdnn_l0.hip: l0_fix_kernel, l0_fix_list_kernel)
constexpr int kFuseCntWords = 8;      // fused soft-max, in-phase tiles: counter words per frame tile (fdnn_gemm.hip:615)
constexpr int kPpoHalfFrames = 160;   // fdnn_ppo.hip: a 320-frame tile is two halves,
constexpr int kPpoCntWords = 4;       // ... each with four counter words (fdnn_ppo.hip:353-354)
constexpr int kChainCtlUsed = 9;      // fdnn_chain.hip:130 (heads 0..7, two 16-byte loads), :548-550 (the leave counter at [8])

struct L0Extent {
  size_t act;                  // bytes of d_act[0]
  size_t cols;                 // columns of the frame image = rows of the digit planes and row constants: must fit xt_ld
  size_t xt, l0park;           // floats
  size_t scr_count, scr_list;  // tiles, list entries
  size_t xd, xstat;            // bytes, floats
  size_t glist, glist_count;
};
// n_rows frames; the context's strides: act_ld, xt_ld (L0Params::n_ld) and the list capacity it passes
inline L0Extent l0_extent(const sel::L0Choice &ch, int D, int H, int h_ld, int j_pad, int n_rows, int act_ld, int xt_ld, int glist_cap) {
  L0Extent e{};
  // every kind stores rows f < n_rows only, H <= act_ld bytes each: fdnn_l0.hip:169 (tile64), :405 (small), :616 (chain),
  // :989 (mfma, screened), :1067 with :1099 / :1142 / :1153 (recomputed outputs: f < n), fdnn_l0s.hip:549 (split)
  e.act = size_t(n_rows) * act_ld;
  const size_t c128 = size_t(n_rows + kL0TileFrames - 1) / kL0TileFrames * kL0TileFrames;
  const size_t node_tiles = size_t(H + kL0TileNodes - 1) / kL0TileNodes;
  switch (ch.kind) {
    case sel::L0Kind::chain:
      // fdnn_l0.hip:682-687: the image kernel covers whole 128-column tiles; :674-676: plane c < 4, row j < j_pad, column < cols
      e.cols = c128;
      e.xt = (4 * size_t(j_pad) - 1) * xt_ld + e.cols;
      // fdnn_l0.hip:519: 32 x 256 float pairs per (frame tile, 128-node tile), the 128-node shape only
      if (ch.tile == 128) e.l0park = (e.cols / 128) * size_t(h_ld / 128) * (32 * 256 * 2);
      break;
    case sel::L0Kind::screened: {
      // fdnn_l0.hip:1202-1205: one counter and one list per (ceil(H / 128), ceil(n_rows / TF)) tile, TF = 128 or 64; :981-983, :1079, :1097
      const int tf = ch.tile == 2 ? 64 : 128;
      e.scr_count = node_tiles * size_t((n_rows + tf - 1) / tf);
      e.scr_list = e.scr_count * kL0ScreenCap;
      break;
    }
    case sel::L0Kind::split:
      // fdnn_l0s.hip:680-683: the pre-pass writes every row a 128-frame matrix tile reads; :186: plane (chunk, digit), 32-row
      // block f / 32 of xt_ld / 32, 1024 bytes a block; :153-155 and :251: three rows of xt_ld constants
      e.cols = c128;
      e.xd = ((size_t(l0_split_chunks(D)) * 3 - 1) * size_t(xt_ld / 32) + e.cols / 32) * 1024;
      e.xstat = 2 * size_t(xt_ld) + e.cols;
      // fdnn_l0s.hip:563-583: entries below glist_cap only; fdnn_l0.hip:1122, :1141; fdnn_l0s.hip:84: two counter words
      e.glist = size_t(glist_cap);
      e.glist_count = 2;
      // fdnn_l0s.hip:570, fdnn_l0.hip:1146-1147, :1223: a counter per 128 x 128 tile, h_ld / 128 a frame tile (no per-tile list)
      e.scr_count = size_t(h_ld / kL0TileNodes) * (e.cols / kL0TileFrames);
      break;
    default: break;  // mfma, small, tile64: the activations only
  }
  return e;
}

struct LayerExtent {
  size_t act_in, act_out;  // bytes of the activation buffer read / written (act_out: hidden layers)
  size_t partial;          // floats (output)
  size_t fuse_s, fuse_cnt, fuse_flag;
  size_t mask_bits;        // words, where the launch packs or reads the context's bit mask
};
// One int8 layer over frames [first, first + n) of the context (hidden layers: first = 0); masked: the call carries a mask
inline LayerExtent layer_extent(const sel::LayerShape &l, const sel::LayerChoice &ch, int first, int n, int act_ld, bool masked = false) {
  LayerExtent e{};
  // QGemmParams::a = row `first`, n_pad rows of lda = act_ld bytes (fdnn_runtime.cpp: prepare_qlayer, run_output): "rows
  // [first + count, first + n_pad) are read as padding frames"
  e.act_in = size_t(first + ch.n_pad) * act_ld;
  if (!l.output) {
    e.act_out = size_t(ch.n_pad) * act_ld;  // whole frame tiles are stored
    return e;
  }
  // fdnn_gemm.hip:1090, fdnn_small.hip:86 / :383 (write), fdnn_kernels.hip:39-40, :144-145 (read): row rows_pad / 64 - 1 at
  // the most, partial_ld floats a row, frames below the in-phase n_pad = partial_ld
  e.partial = size_t(l.rows_pad / kPartialNodes) * ch.partial_ld;
  if (ch.form == sel::Form::ppo) {
    // fdnn_ppo.hip:286-291: frame pairs below n_pad / 320; :311: half e_half < 2 pairs; :352: kMT x kHT sums a half; :353-354
    const size_t halves = 2 * size_t(ch.n_pad / sel::kPpFrameTile);
    e.fuse_s = halves * sel::kPpoNodeTiles * kPpoHalfFrames;
    e.fuse_cnt = halves * kPpoCntWords;
  } else if (ch.fused) {
    // fdnn_gemm.hip:614-615, :638: frame tile nt < n_pad / FT, node tile mt < MT = rows_pad / 256; :778, :788, :820: a flag per (nt, mt)
    const size_t tiles = size_t(ch.n_pad / ch.frame_tile), mt = size_t(l.rows_pad / 256);
    e.fuse_s = tiles * mt * ch.frame_tile;
    e.fuse_cnt = tiles * kFuseCntWords;
    e.fuse_flag = tiles * mt;
  }
  if (masked && ch.mask_bits) e.mask_bits = size_t(n) * size_t((l.rows + 63) / 64);  // launch_mask_pack: [n][ceil(rows / 64)]
  return e;
}

struct ChainExtent {
  size_t act;  // bytes, of either activation buffer
  size_t ctl, done;
};
// One chained launch of n_layers hidden layers (fdnn_chain.hip)
inline ChainExtent chain_extent(const sel::HiddenPlan &p, int n_layers, int act_ld) {
  ChainExtent e{};
  e.act = size_t(p.n_pad) * act_ld;
  e.ctl = kChainCtlUsed;
  // fdnn_chain.hip:111-119: frame tile gnt < NT = n_pad / FT; :263, :524: done + gnt * n_layers + layer
  e.done = size_t(p.n_pad / p.frame_tile) * n_layers;
  return e;
}

}  // namespace fdnn
