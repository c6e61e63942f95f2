// fdnn_kernels.hpp -- launch interface of the gfx950 kernels (fdnn_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "fdnn_ctx_layout.hpp"  // kMaxFrameTile, kPartialNodes, kL0ScreenCap, l0_split_plane_bytes
#include "fdnn_note.hpp"
#include "fdnn_select.hpp"
#include "fdnn_lists_union.hpp"
#include "fdnn_set.hpp"
#include "fdnn_sets.hpp"
#include "fdnn_topk.hpp"
#include "fdnn_pool.hpp"
#include "fdnn_loglik.hpp"
#include "fdnn_align.hpp"
#include "fdnn_align_graph.hpp"
#include "fdnn_fb.hpp"

// Run-time switches.  The DEPLOYMENT switches (FDNN_BATCHER, FDNN_DEVICES, FDNN_FUSE_NORM,
// FDNN_GROUP_*, FDNN_JNI_KEEP_MB, FDNN_CHAIN, FDNN_CHUNK_FRAMES) are read with std::getenv; those that bear on which kernel
// runs, in one place (fdnn_select.cpp, into fdnn_select.hpp's Tuning).  Everything else -- tile-shape
// overrides, thresholds and kernel choices that the sweeps under tools/ turn -- exists only in measurement builds
// (-DFDNN_ABLATION: tools/build_variant.sh): in the shipped library FDNN_TUNE_ENV is a null pointer, the defaults are
// constants, and the compile-time ablation branches (FDNN_GEMM_DEBUG, FDNN_L0S_DEBUG, FDNN_CHAIN_CLK, ...) cannot be set.
#ifdef FDNN_ABLATION
#include <cstdlib>
#define FDNN_TUNE_ENV(name) std::getenv(name)
#else
#define FDNN_TUNE_ENV(name) static_cast<const char *>(nullptr)
#if (defined(FDNN_GEMM_DEBUG) && FDNN_GEMM_DEBUG) || (defined(FDNN_L0S_DEBUG) && FDNN_L0S_DEBUG) || (defined(FDNN_L0_DEBUG) && FDNN_L0_DEBUG) || \
    (defined(FDNN_CHAIN_CLK) && FDNN_CHAIN_CLK) || defined(FDNN_L0S_CLK) || defined(FDNN_GEMM_PAD)
#error "ablation / clock builds need -DFDNN_ABLATION (tools/build_variant.sh)"
#endif
#endif

namespace fdnn {

// Layer 0: shift/scale + fp32 affine + bias + sigmoid LUT -> s8 activations.
struct L0Params {
  const float *x;      // [n][D] caller frames (never written)
  const float *shift;  // [D]
  const float *scale;  // [D]
  const float *w;      // [H][D]
  const float *bias;   // [H]
  const uint8_t *lut;  // [kLutExt] XOR 0x80
  int8_t *act_out;     // [n_rows][act_ld]
  int act_ld;          // row stride of act_out (H padded to the GEMM k-step)
  float *tap_lin;      // [n][H] or null
  int n, D, H;
  int n_rows;          // rows of act_out to fill (>= n, the next GEMM's padded frame count)
  int fma;             // 0: mul then add (canonical), 1: fused
  int kernel;          // canonical flavour: 0 pick by batch size, 1 chain-pass kernel, 2 64 x 64-tile kernel
  // canonical flavour: chain-major operand images  img[(c + 2) % 4][j][col] = src[col][4j + c]
  float *xt;           // [4][j_pad][n_ld] frame image, scratch, rewritten by every launch
  const float *wt;     // [4][j_pad][h_ld] weight image (launch_l0_weight_image at model load)
  float *park;         // [n_ld/128][h_ld/128][64 KB] scratch: l2 + l3 of a tile while l0, l1 run (128-node tiles only, else null)
  int j_pad, jc;       // D/4 rounded up to the chunk depth jc = l0_chunk_rows(D)
  int n_ld, h_ld;      // image row lengths: frame capacity and H, both rounded up to 128
  // canonical flavour, screened path (large batches, no taps): the FUSED chains on the fp32 MFMA for every output,
  // a rigorous bound on |fused - unfused| per output, and the exact unfused chains for the few outputs whose
  // table index the difference could change (fdnn_l0.hip: "screened").  All null/0 = path not available.
  const float *wnorm;  // [H] upper bound of ||w_n||_2 (model load)
  uint32_t *scr_count; // [tiles] flagged outputs per 128 x 128 tile; zero between launches
  uint16_t *scr_list;  // [tiles][kL0ScreenCap] tile-local indices frame_row * 128 + node_col
  unsigned long long *scr_stats;  // [2] running totals: outputs screened, outputs recomputed (may be null)
  // round 4, the screening on the INT8 matrix pipe (fdnn_l0s.hip): 24-bit integer images of both operands as three
  // int8 digit planes in MFMA fragment order + per-row constants of the error bound.  All null = path not available.
  int8_t *xd;          // [chunks][3][n_ld / 32][1024] frame planes, scratch, rewritten by every launch
  float *xstat;        // [3][n_ld]: 2^16 / c_f, ||x_f||_2 (rounded up), a_f
  const int8_t *wd;    // [chunks][3][h_ld / 32][1024] node planes (model load)
  const float *wstat;  // [3][h_ld]: 2^8 / c_n, ||w_n||_2 (rounded up), 2^8 b_n
  uint2 *glist;        // [glist_cap] {frame, node} of every flagged output of the launch (tiles append with one atomic each)
  uint32_t *glist_count;  // [2]: entries appended; tiles that overflowed into the whole-tile path.  Zeroed by the pre-pass
  int glist_cap;
  const uint32_t *luthalf;  // [kLut2Size (+pad)] the half-step table, 4 bytes per entry: table byte + the 'same byte across the boundary' gate
  // parity tests only (fdnn_debug_layer0_screen; null in production): what the int8 screening saw per output, [n][H] each --
  // t~ = 100 lin~ and the half-width Dd of the interval it vouches for; |100 lin_ref - t~| <= Dd is the bound's claim
  float *dbg_t;
  float *dbg_dd;
};
void launch_l0(const L0Params &p, const sel::L0Choice &ch, hipStream_t s);  // ch = sel::choose_l0
// fdnn_l0s.hip: the node half (host code, model load); pre-pass + matrix kernel
// (launch_l0 follows with the exact recomputation of the flagged outputs)
void launch_l0_split(const L0Params &p, int wn_cfg, hipStream_t s);
void l0_split_build_weights(const float *w, const float *wnorm, const uint8_t *lut2, int H, int D, int h_ld, std::vector<int8_t> *planes,
                            std::vector<float> *stat, std::vector<uint32_t> *half);
int l0_chunk_rows(int D);
void launch_l0_weight_image(const float *w, float *wt, int H, int D, int j_pad, int h_ld, hipStream_t s);

// int8 layer: C[node][frame] = sum_k W[node][k] * (A[frame][k] + 128), then the
// layer's epilogue.  W rows are padded to 256, A rows to the frame tile.
struct QGemmParams {
  const int8_t *w;        // [rows_pad][K]  (K = padded input width, pad columns are zero)
  const int8_t *a;        // [n_pad][K]  s8 = u8 - 128 (pad columns: anything)
  const float *bias;      // [rows_pad]
  const int32_t *wsum;    // [rows_pad]  128*sum_k w
  const int32_t *fix_grp; // [rows_pad/64 + 1] entry range of every 64-node group
  const void *fix_ent;    // FixEntry[n_fix] sorted by node; null when the layer has no risky pairs
  const uint8_t *lut;     // [kLutExt]
  const uint8_t *lut2;    // [kLut2Size] half-step table (fast epilogue)
  int rows, rows_pad, K, n, n_pad;
  int ldw, lda;           // row strides (bytes) of w and a: K plus the anti-channel-conflict skew
  int frame_tile;         // 32 / 64 / 128 / 160 / 256 / 320, n_pad is a multiple of it
  int small;              // 1: the small-batch kernel (fdnn_small.hip; frame_tile = 32)
  int node_tile;          // 256 (default) or 128: with frame_tile 128, the 128 x 128 four-wave shape for mid-size batches
  int debug;              // timing experiments only (FDNN_GEMM_DEBUG): 1 no staging, 2 no MFMA, 4 no LDS reads
  float coef, rcp_coef;
  int fastdiv;
  // hidden-layer output
  int8_t *act_out;        // [n_pad][act_ld]
  int act_ld;
  // output-layer output
  float *out;             // [n][rows] un-normalised exp, row stride = rows
  float *partial;         // [rows_pad/kPartialNodes][partial_ld]
  int partial_ld;
  const int8_t *mask;     // [n][rows] or null (lazy contract)
  const uint64_t *mask_bits;  // [n][mask_wpr] the same mask, one bit per node (launch_mask_pack), or null: the large-batch
  int mask_wpr;               // production instances read one 64-bit word per frame row and 64-node group instead of 64 bytes
  // fused soft-max (large-batch dense output instance): where the probabilities go, the per-tile row sums S
  // [n_pad / frame_tile][rows_pad / 256][frame_tile], the per-frame-tile {arrived, left} counters (zero between launches)
  // and the per-tile "gave up waiting" flags (the frame tile's last workgroup scales such blocks); all null = the unfused path
  float *final;
  float *fuse_s;
  uint32_t *fuse_cnt;
  uint32_t *fuse_flag;
  int fuse_stagger;       // fused soft-max: start delay of the first round's frame tile j = (j % 8) * this many 512-cycle naps (see qgemm_kernel)
  unsigned long long *fuse_giveups;  // per model: tiles that had to be scaled after the fact (a workgroup gave up waiting); null = not counted
  unsigned long long *fuse_fault;    // per model, HOST memory: raised with the first give-up -- the host then stops fusing for this model (run_output); null = nobody listens
  // accumulator probe of the PRODUCTION output instances (parity tests only; null otherwise): the int32 accumulators of
  // every probe_stride-th frame, [ceil(n / probe_stride)][rows] -- a wave-uniform branch in front of the epilogue
  int32_t *acc_probe;
  int probe_stride;
  // taps (null in production)
  int32_t *tap_acc;       // [n][rows]
  float *tap_logit;       // [n][rows]
};
// The launchers take what sel::choose_layer chose (fdnn_select.hpp) and the CU count of the model's device where the
// grid depends on it.  Small batches (fdnn_small.hip; ntm: 32- or 64-node tiles), the tiled shapes (fdnn_gemm.hip):
void launch_qgemm_small_hidden(const QGemmParams &p, int ntm, hipStream_t s);
void launch_qgemm_small_output(const QGemmParams &p, hipStream_t s);
void launch_qgemm_hidden(const QGemmParams &p, GemmShape shape, hipStream_t s);
void launch_qgemm_output(const QGemmParams &p, GemmShape shape, hipStream_t s);

// An int8 hidden layer of a large batch with the two waves of every SIMD in different roles (fdnn_pp.hip): one computes
// (fragment reads + MFMAs only) while its partner stages that tile's operands and runs the epilogue of the tile it computed
// before.  256-node x 320-frame tiles (n_pad a multiple of sel::kPpFrameTile), K = 2048, validated 3-operation division.
void launch_qpp_hidden(const QGemmParams &p, int n_cu, hipStream_t s);
// fdnn_ppo.hip: the same role split for the OUTPUT layer of a large dense batch, soft-max scaled inside the kernel (the
// caller holds the device's chain of fused launches: run_output)
void launch_qppo_output(const QGemmParams &p, int n_cu, hipStream_t s);

// The int8 HIDDEN layers of a pass in one persistent launch (fdnn_chain.hip): tasks (layer, frame tile, node tile) drawn
// from per-XCD queues, a task waits only for its own frame tile's node tiles of the layer before.  All hidden layers of
// a net have the same shape (README.md:10), so one set of sizes serves every layer.
struct QChainLayer {
  const int8_t *w;         // [rows_pad][ldw]
  const float *bias;       // [rows_pad]
  const int32_t *wsum;     // [rows_pad]
  const int32_t *fix_grp;  // as QGemmParams
  const void *fix_ent;     // null: no risky pairs in this layer
  float coef, rcp_coef;
};
struct QChainParams {
  QChainLayer layer[kMaxChainLayers];
  int n_layers;
  int8_t *act[2];          // layer i reads act[i & 1] and writes act[(i & 1) ^ 1]; rows [n_pad][lda]
  const uint8_t *lut2;     // half-step sigmoid table
  int rows, rows_pad, K, ldw, lda, n, n_pad;
  int frame_tile;          // 320 or 256
  uint32_t *ctl;           // [16]: queue heads [0..7], workgroups that have left [8]; zero between launches
  uint32_t *done;          // [n_pad / frame_tile][n_layers] node tiles finished; zero between launches
  unsigned long long *faults;  // waits that ran into their bound (never in a healthy setup): counted, fdnn_model_chain_faults
  unsigned long long *fault_flag;  // host-visible word of the launching context, raised with the count (null: not raised)
  long long *clk;          // measurement builds (FDNN_CHAIN_CLK): [8 + clk_cap * 10] phase clocks per task, else null
  int clk_cap;
};
void launch_qchain(const QChainParams &p, int n_cu, hipStream_t s);

// Lazy output by active-node lists (fdnn_lists.hip; the lists' contract and the per-node pair index: fdnn_lists.hpp):
// score writes e = exp(z) of every entry into probs, finish scales each row's entries in place and writes its 1 / total.
struct ListsParams {
  const int8_t *w;            // [rows_pad][ldw] the output layer's int8 rows (pad columns zero)
  const int8_t *a;            // [count][lda] s8 last-hidden activations of the call's rows (pad columns: anything)
  const float *bias;          // [rows_pad]
  const int32_t *wsum;        // [rows_pad] 128 * sum_k w
  const int32_t *fix_off;     // [rows + 1] a node's saturating pairs in fix_pairs; both null: the layer has none
  const uint32_t *fix_pairs;  // k | w0 << 16 | w1 << 24
  const int32_t *row_ptr;     // [count + 1]; null (finish only): every row has row_len entries, row r at r * row_len
  const int32_t *nodes;       // [nnz]
  float *probs;               // [nnz]
  float *inactive;            // [count]
  int32_t *acc;               // [nnz] the int32 accumulators as the score kernel holds them (parity tests), or null
  int rows, K, ldw, lda, count, nnz;
  int row_len;                // the uniform row length of a shared node set (fdnn_set.hip), with row_ptr null
  int epg;                    // consecutive entries one 16-lane group scores (lists_entries_per_group)
  float coef, rcp_coef;
  int fastdiv;
};
void launch_lists_score(const ListsParams &p, hipStream_t s);
void launch_lists_finish(const ListsParams &p, hipStream_t s);
int lists_entries_per_group(long long nnz, int n_cu);
void lists_launch_counts(unsigned long long out[3]);  // launches so far: score without / with the pair walk, finish

// Lazy output for a shared node set (fdnn_set.hip; the guard and the tile plan: fdnn_set.hpp): e = exp(z) of (row r, entry j)
// into probs[r * len + j] on the int8 MFMA; launch_lists_finish with row_ptr null and row_len = len then owns the total.
struct SetParams {
  const int8_t *w;            // [rows][ldw] the output layer's int8 rows (pad columns zero)
  const int8_t *a;            // [count][lda] s8 last-hidden activations of the call's rows
  const float *bias;          // [rows_pad]
  const int32_t *wsum;        // [rows_pad] 128 * sum_k w
  const int32_t *fix_off;     // [rows + 1] a node's saturating pairs in fix_pairs; both null: the layer has none
  const uint32_t *fix_pairs;  // k | w0 << 16 | w1 << 24
  const int32_t *nodes;       // [len] the set (not validated: fdnn_set.hpp's guard)
  float *probs;               // [count][len]
  int32_t *acc;               // [count][len] the int32 accumulators as the kernel holds them (parity tests), or null
  int rows, K, ldw, lda, count, len;
  float coef, rcp_coef;
  int fastdiv;
  set::Plan plan;             // set::plan(count, len, CUs)
};
void launch_set_score(const SetParams &p, hipStream_t s);
// The fallback (a layer the MFMA kernel's shape does not apply to, fdnn_debug_set_kernel(2)): the set as lists for the
// list kernels -- row_ptr[r] = r * len for r in [0, count], rep[r * len + j] = nodes[j].  Counted as set_launch_counts[2].
void launch_set_expand(const int32_t *nodes, int len, int count, int32_t *row_ptr, int32_t *rep, hipStream_t s);
void set_launch_counts(unsigned long long out[3]);  // MFMA kernel without / with the pair walk, calls served by the list kernels
int set_kernel_mode();                              // fdnn_debug_set_kernel: 0 the default rule, 1 MFMA where its shape applies, 2 fallback
void set_kernel_mode(int mode);

// Lazy output for per-segment node sets (fdnn_sets.hip; tables, launches and slices: fdnn_sets.hpp): the set kernel's tile on
// up to sets::kMaxSegs segments in one launch.  p carries the layer and a / nodes / probs / acc of the call's first row,
// whole node array and first block (its count, len and plan are not read); l is passed to the kernel by value.
// launch_lists_finish with the call's synthesized row_ptr then owns the totals.  fdnn_debug_set_kernel's mode applies.
void launch_sets_score(const SetParams &p, const sets::Launch &l, hipStream_t s);
// row_ptr[row0_s + r] = out_off_s + r * len_s for the launch's segments (sets::row_ptr), row_set[row0_s + r] = set_off_s
// unless row_set is null (sets::row_set), and row_ptr[end_row] = end unless end_row < 0 (the call's last launch).
void launch_sets_rows(const sets::Launch &l, int32_t *row_ptr, int32_t *row_set, int end_row, int end, hipStream_t s);
// The fallback: the sets as lists for the list kernels -- rep[row_ptr[r] + j] = nodes[row_set[r] + j] for every row r of
// the call (sets::row_ptr, sets::row_set, both on the device).  Counted as sets_launch_counts[2], once per call.
void launch_sets_expand(const int32_t *nodes, const int32_t *row_ptr, const int32_t *row_set, int count, int32_t *rep, hipStream_t s);
void sets_launch_counts(unsigned long long out[3]);  // MFMA launches without / with the pair walk, calls served by the list kernels

// Lazy output by lists over per-frame-group node unions (fdnn_lists_union.hip; groups, buffers and the grid bound:
// fdnn_lists_union.hpp).  build writes u_nodes / pos / u_len / work / counter from the caller's lists (and the NaN of an
// entry whose node is outside the layer); score runs the set kernels' tile on every work item -- p carries the layer, a
// and lda of the call's first row (its nodes, probs, acc, count, len and plan are not read) -- and gathers the listed
// entries' e into probs; launch_lists_finish over the caller's row_ptr then owns the totals.
struct UnionParams {
  const int32_t *row_ptr;  // [count + 1] the caller's (not validated: values are clamped to [0, nnz])
  const int32_t *nodes;    // [nnz] the caller's (not validated: set::node_ok before any use)
  float *probs;            // [nnz]
  int32_t *acc;            // [nnz] the int32 accumulators as the tile holds them (parity tests), or null
  int32_t *u_nodes, *pos, *u_len, *work, *counter;  // lunion::Layout
  int rows, count, nnz, group_tiles, bound;
};
hipError_t launch_lists_union_build(const UnionParams &u, int n_groups, hipStream_t s);  // zeroes the counter first
void launch_lists_union_score(const SetParams &p, const UnionParams &u, int n_cu, hipStream_t s);
void lists_union_note_fallback();  // a call with the switch on that the list kernels serve
void lists_union_launch_counts(unsigned long long out[4]);  // build, score without / with the pair walk, fallback calls

// The dense output with a top-k return (fdnn_topk.hip; the order, the plan and the host restatement: fdnn_topk.hpp): of every
// row of rows [n][width] the k first-ranked nodes and their values into nodes / vals [n][k].  The caller has checked
// topk::args_ok(width, k).  The form is the plan's under fdnn_debug_set_topk_kernel's mode.
void launch_topk(const float *d_rows, int n, int width, int k, int32_t *d_nodes, float *d_vals, hipStream_t s);
void topk_launch_counts(unsigned long long out[2]);  // launches so far: resident form, streaming form
int topk_kernel_mode();                              // fdnn_debug_set_topk_kernel: 0 the plan's rule, 1 resident where the width allows, 2 streaming
void topk_kernel_mode(int mode);

// The dense output pooled over a node -> class map (fdnn_pool.hip; the map, the order of the additions, the plan and the host
// restatement: fdnn_pool.hpp): of every row [width] of d_rows [n] the sums over the classes of the CSR d_class_ptr
// [n_classes + 1], d_member [nnz] (as pool::build_csr makes it) into d_out [n][n_classes].  No-op unless n > 0.  The form is
// the plan's under fdnn_debug_set_pool_kernel's mode.
void launch_pool(const float *d_rows, int n, int width, const int32_t *d_class_ptr, const int32_t *d_member, int n_classes, float *d_out, hipStream_t s);
void pool_launch_counts(unsigned long long out[2]);  // launches so far: resident form, streaming form
int pool_kernel_mode();                              // fdnn_debug_set_pool_kernel: 0 the plan's rule, 1 resident where the width allows, 2 streaming
void pool_kernel_mode(int mode);

// The dense output as decoder scores (fdnn_loglik.hip; the logarithm, the score, the plan and the host restatement:
// fdnn_loglik.hpp): of every row [width] of d_rows [n] ln(p_i) - d_log_prior[i], floored, into d_out [n][width] of fp32
// (type loglik::kF32) or fp16 (kF16).  Entries: of (d_nodes[j], d_p[j]) the same with the node's prior into d_out [count]; a
// node outside [0, width) gives a NaN.  No-ops unless n / count > 0.  The rows' form is the plan's under
// fdnn_debug_set_loglik_kernel's mode.
void launch_loglik_rows(const float *d_rows, int n, int width, const float *d_log_prior, float floor, int type, void *d_out, hipStream_t s);
void launch_loglik_entries(const int32_t *d_nodes, const float *d_p, long long count, int width, const float *d_log_prior, float floor, int type, void *d_out, hipStream_t s);
void loglik_launch_counts(unsigned long long out[3]);  // launches so far: rows vector form, rows scalar form, entries
int loglik_kernel_mode();                                // fdnn_debug_set_loglik_kernel: 0 the plan's rule, 1 vector where allowed, 2 scalar
void loglik_kernel_mode(int mode);

// Forced alignment (fdnn_align.hip; the emission, the step, the plan and the host restatement: fdnn_align.hpp): the launches
// of a plan (align::plan over the call's host tables) over device-resident rows.  type: loglik::kF32 / kF16 -- the rows are
// probabilities, d_state_node [states] and d_log_prior [width] make the scores -- or align::kScores -- the rows are scores,
// d_state_node and d_log_prior are not read.  d_self_lp / d_next_lp may be null (+0).  d_scratch: p.scratch_words 32-bit
// words on an 8-byte boundary (null when there are none).  d_path [sum of T] int32, d_total [n_segs].
struct AlignArgs {
  const float *d_rows = nullptr;
  const int32_t *d_col = nullptr, *d_state_node = nullptr;
  const float *d_log_prior = nullptr;
  int width = 0;
  float floor = 0.0f;
  int type = align::kScores;
  const float *d_self_lp = nullptr, *d_next_lp = nullptr;
  uint32_t *d_scratch = nullptr;
  int32_t *d_path = nullptr;
  float *d_total = nullptr;
};
void launch_align(const align::Plan &p, const AlignArgs &a, hipStream_t s);
void align_launch_counts(unsigned long long out[2]);  // launches so far: wave form, workgroup form
int align_kernel_mode();                               // fdnn_debug_set_align_kernel: 0 the plan's rule, 1 wave where allowed, 2 workgroup
void align_kernel_mode(int mode);

// Alignment graphs (fdnn_align_graph.hip; the step, the plan and the host restatement: fdnn_align_graph.hpp): the launches of
// a plan (align_graph::plan over the call's host tables) over device-resident rows.  rows, type, d_col, d_state_node,
// d_log_prior as AlignArgs.  d_arc_ptr [states + 1], d_arc_src, d_arc_lp [arcs]: device copies of the host tables the plan was
// made from (the plan's counts bound every arc index).  d_start_lp / d_final_lp [states] may be null (state 0 / the last
// state).  d_scratch: p.scratch_words 32-bit words (null when there are none).  d_path [sum of T] int32, d_total [n_segs].
struct AlignGraphArgs {
  const float *d_rows = nullptr;
  const int32_t *d_col = nullptr, *d_state_node = nullptr;
  const float *d_log_prior = nullptr;
  int width = 0;
  float floor = 0.0f;
  int type = align::kScores;
  const int32_t *d_arc_ptr = nullptr, *d_arc_src = nullptr;
  const float *d_arc_lp = nullptr, *d_start_lp = nullptr, *d_final_lp = nullptr;
  uint32_t *d_scratch = nullptr;
  int32_t *d_path = nullptr;
  float *d_total = nullptr;
};
void launch_align_graph(const align_graph::Plan &p, const AlignGraphArgs &a, hipStream_t s);
void align_graph_launch_counts(unsigned long long out[2]);  // launches so far: wave form, workgroup form
int align_graph_kernel_mode();  // fdnn_debug_set_align_graph_kernel: 0 the plan's rule, 1 wave where allowed, 2 workgroup
void align_graph_kernel_mode(int mode);

// Alignment graphs, summed (fdnn_fb.hip; the two stated functions, the recursion, the plan and the host restatement:
// fdnn_fb.hpp): the launches of a plan (fb::plan over the call's host tables) over device-resident rows -- every launch
// forward, then, where d_gamma is not null, every launch backward.  rows, type, d_col, d_state_node, d_log_prior, the arc
// tables and d_start_lp / d_final_lp as AlignGraphArgs.  d_t_ptr [states + 1], d_t_src, d_t_lp [arcs]: device copies of the
// transposed tables (fb::transpose), read only when d_gamma is not null.  d_scratch: p.scratch_words fp32 words, the
// lattice (null when there are none).  d_total [n_segs], d_gamma [p.gamma_words] or null: forward only.
struct FbArgs {
  const float *d_rows = nullptr;
  const int32_t *d_col = nullptr, *d_state_node = nullptr;
  const float *d_log_prior = nullptr;
  int width = 0;
  float floor = 0.0f;
  int type = align::kScores;
  const int32_t *d_arc_ptr = nullptr, *d_arc_src = nullptr;
  const float *d_arc_lp = nullptr, *d_start_lp = nullptr, *d_final_lp = nullptr;
  const int32_t *d_t_ptr = nullptr, *d_t_src = nullptr;
  const float *d_t_lp = nullptr;
  float *d_scratch = nullptr;
  float *d_total = nullptr, *d_gamma = nullptr;
};
void launch_fb(const fb::Plan &p, const FbArgs &a, hipStream_t s);
// out[i] = exp_neg(a[i]) (op 0) or ladd(a[i], b[i]) (op 1): the stated functions in a trivial kernel (fdnn_debug_fb_math_device)
void launch_fb_math(int op, const float *d_a, const float *d_b, float *d_out, long long n, hipStream_t s);
void fb_launch_counts(unsigned long long out[4]);  // launches so far: forward wave, forward workgroup, backward wave, backward workgroup
int fb_kernel_mode();  // fdnn_debug_set_fb_kernel: 0 the plan's rule, 1 wave where allowed, 2 workgroup
void fb_kernel_mode(int mode);

// bits[f][w] bit b = mask[f][64 w + b] != 0  (words per row = ceil(rows / 64); bits past the row are zero).  The lazy
// contract's byte masks (80 MB for 10 000 frames x 8000 nodes) are read once here, at HBM speed, instead of inside the
// output GEMM's epilogue.
void launch_mask_pack(const int8_t *mask, uint64_t *bits, int n, int rows, hipStream_t s);
void launch_mask_unpack(const uint64_t *bits, int8_t *mask, int n, int rows, hipStream_t s);
// comp[f][0] = row f's inactive value, comp[f][1 + r] = probability of its r-th active node (rows of `stride` floats)
void launch_lazy_compact(const float *out, const uint64_t *bits, float *comp, int n, int rows, int stride, hipStream_t s);

// dst[f][:] = out[f][:] / sum_t partial[t][f]   (dst == out: in place; dst may be host-mapped)
void launch_normalize(float *out, float *dst, const float *partial, int n, int partial_ld, int rows, int n_partial, hipStream_t s);

// Exhaustive check of the 3-op division against IEEE division for every int32
// accumulator in the closed range [-bound, bound]; the caller passes the
// layer's own bound, (cols_pad / 2) * 32768 (each adjacent pair saturates to
// int16).  *d_mismatch receives the count of accumulators that differ.
void launch_fastdiv_check(float coef, float rcp, long long bound, unsigned long long *d_mismatch, hipStream_t s);

// s8 <-> u8 view of activations for taps / read-back.
void launch_xor80(const int8_t *in, uint8_t *out, size_t count, hipStream_t s);

// Splicing raw feature frames into rows (fdnn_splice.hip).  Passed by value: the offsets and the launch's segment table are
// kernel arguments (1.8 KB).  Segment g covers rows [seg_row[g], seg_row[g + 1]); its row t reads the raw frames
// clamp(seg_center[g] + (t - seg_row[g]) + o, seg_lo[g], seg_hi[g]) of the raw buffer, one per offset o.
constexpr int kSpliceMaxOffsets = 64;
constexpr int kSpliceMaxSegs = 96;  // per launch: longer tables go as several launches
struct SpliceArgs {
  int offsets[kSpliceMaxOffsets];
  int count, raw_dim, input_dim, n_segs;
  int seg_row[kSpliceMaxSegs], seg_center[kSpliceMaxSegs], seg_lo[kSpliceMaxSegs], seg_hi[kSpliceMaxSegs];
};
// rows [row0, row0 + rows) into x[rows][input_dim] (x holds row row0 first); raw [raw_frames][raw_dim]
void launch_splice(const float *raw, int raw_frames, float *x, int row0, int rows, const SpliceArgs &a, hipStream_t s);
// The same rows [0, rows) from a segment table in DEVICE memory, one launch whatever its length (a live batch of the scoring
// loop: one segment per push): d_segs [n_segs][4] = (row, center, lo, hi), 16-byte aligned; d_row_seg [rows], each row's
// segment index.  Only the offsets travel as kernel arguments.  Counted by splice_table_counts, not by the launch recorder.
struct SpliceOffsets {
  int offsets[kSpliceMaxOffsets];
  int count, raw_dim, input_dim;
};
void launch_splice_table(const float *raw, int raw_frames, float *x, int rows, const int32_t *d_segs, const int32_t *d_row_seg, int n_segs,
                         const SpliceOffsets &a, hipStream_t s);
void splice_table_counts(unsigned long long *launches, unsigned long long *max_segs);  // process-wide: launches, the longest table

}  // namespace fdnn
