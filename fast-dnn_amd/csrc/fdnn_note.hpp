// fdnn_note.hpp -- the launch recorder: one stable name per host launch branch of a compute kernel, a process-wide
// count per name.  Off by default: a launcher then pays at most one relaxed load per kernel it starts (note_launch).  The names say which BRANCH a
// launcher took, not which template symbol it started: two branches that start the same instantiation are one name.
// The table is static, so it can be listed without a device (fdnn_debug_launch_name); the tests' ledger
// (tests/dispatch_ledger.py) must cover every name in it: a new launch branch needs a name here and a case there.
//
// Not in the table yet: the two kernels of lazy output by lists (fdnn_lists.hip: score with / without the pair walk, finish).
// They are counted by a counter of their own (fdnn_debug_lists_launches) because every name here needs a ledger case; a
// later change that adds those cases can fold them in as "lists.score.fix", "lists.score.nofix" and "lists.finish".
// Likewise the kernel of lazy output for a shared node set (fdnn_set.hip: with / without the pair walk) and its fallback to
// the list kernels: fdnn_debug_set_launches counts them; as names they would be "set.score.fix", "set.score.nofix" and
// "set.fallback" (the set path's finish launch is the list path's and is counted there).
// And the segmented form of that kernel (fdnn_sets.hip: one set per segment, up to 64 segments in a launch): counted by
// fdnn_debug_sets_launches, apart from the set kernel's counter; as names "sets.score.fix", "sets.score.nofix" and
// "sets.fallback".  Its row-pointer and list-writing helpers are not counted: they score nothing.
// And the union path of the list calls (fdnn_lists_union.hip, fdnn_model_set_lists_union): counted by
// fdnn_debug_lists_union_launches; as names "lists.union.build", "lists.union.score.nofix", "lists.union.score.fix" and
// "lists.union.fallback" (its finish launch is the list path's and is counted there).
// And the two kernels that run BEHIND a dense pass on its finished rows, the top-k selection (fdnn_topk.hip:
// fdnn_debug_topk_launches) and the class pooling (fdnn_pool.hip: fdnn_debug_pool_launches), each counted by form; as names
// "topk.resident", "topk.streaming", "pool.resident" and "pool.streaming".  The decoder scores (fdnn_loglik.hip:
// fdnn_debug_loglik_launches) likewise: "loglik.rows.vector", "loglik.rows.scalar" and "loglik.entries".
// And the splice of a scoring-loop batch with a live piece, whose segment table is read from device memory (fdnn_splice.hip,
// splice_table_kernel): counted by fdnn_debug_live_launches; as a name "splice.table".
#pragma once
#include <atomic>

#include "fdnn_select.hpp"

namespace fdnn {

// (GemmShape, the tile shapes of launch_qgemm: fdnn_select.hpp)
// branches of launch_cfg
enum GemmBranch {
  gb_tap, gb_prod, gb_prod_nofix, gb_plain, gb_anyw, gb_masked, gb_masked_anyw, gb_fused, gb_fused_masked, gb_fused_anyw, gb_fused_masked_anyw, gb_fused_nofix, gb_fused_masked_nofix, gb_count
};

// G(output layer, shape, branch, name, ablation-only): the instances of fdnn_gemm.hip -- launch_cfg compiles exactly these
// (92 rows, 23 of them in measurement builds only; with the 63 names below: 155, 33 of them ablation-only)
#define FDNN_GEMM_LAUNCH_NAMES(G) \
  G(0, tdiv, tap, "gemm.hid.tdiv.tap", 0) \
  G(0, tdiv, prod, "gemm.hid.tdiv.prod", 0) \
  G(1, tdiv, tap, "gemm.out.tdiv.tap", 0) \
  G(1, tdiv, plain, "gemm.out.tdiv.plain", 0) \
  G(1, tdiv, anyw, "gemm.out.tdiv.anyw", 0) \
  G(1, tdiv, masked, "gemm.out.tdiv.masked", 0) \
  G(1, tdiv, masked_anyw, "gemm.out.tdiv.masked_anyw", 0) \
  G(0, ft32w1, tap, "gemm.hid.ft32.w1.tap", 0) \
  G(0, ft32w1, prod, "gemm.hid.ft32.w1.prod", 0) \
  G(0, ft32, tap, "gemm.hid.ft32.tap", 0) \
  G(0, ft32, prod, "gemm.hid.ft32.prod", 0) \
  G(1, ft32, tap, "gemm.out.ft32.tap", 0) \
  G(1, ft32, plain, "gemm.out.ft32.plain", 0) \
  G(1, ft32, anyw, "gemm.out.ft32.anyw", 0) \
  G(1, ft32, masked, "gemm.out.ft32.masked", 0) \
  G(1, ft32, masked_anyw, "gemm.out.ft32.masked_anyw", 0) \
  G(0, ft64, tap, "gemm.hid.ft64.tap", 0) \
  G(0, ft64, prod, "gemm.hid.ft64.prod", 0) \
  G(1, ft64, tap, "gemm.out.ft64.tap", 0) \
  G(1, ft64, plain, "gemm.out.ft64.plain", 0) \
  G(1, ft64, anyw, "gemm.out.ft64.anyw", 0) \
  G(1, ft64, masked, "gemm.out.ft64.masked", 0) \
  G(1, ft64, masked_anyw, "gemm.out.ft64.masked_anyw", 0) \
  G(0, ft128nt128, tap, "gemm.hid.ft128.nt128.tap", 0) \
  G(0, ft128nt128, prod, "gemm.hid.ft128.nt128.prod", 0) \
  G(0, ft128bk128, prod, "gemm.hid.ft128.bk128.prod", 0) \
  G(1, ft128bk128, plain, "gemm.out.ft128.bk128.plain", 0) \
  G(1, ft128bk128, anyw, "gemm.out.ft128.bk128.anyw", 0) \
  G(1, ft128bk128, masked, "gemm.out.ft128.bk128.masked", 0) \
  G(1, ft128bk128, masked_anyw, "gemm.out.ft128.bk128.masked_anyw", 0) \
  G(1, ft128bk128, fused, "gemm.out.ft128.bk128.fused", 0) \
  G(1, ft128bk128, fused_masked, "gemm.out.ft128.bk128.fused_masked", 0) \
  G(1, ft128bk128, fused_anyw, "gemm.out.ft128.bk128.fused_anyw", 0) \
  G(1, ft128bk128, fused_masked_anyw, "gemm.out.ft128.bk128.fused_masked_anyw", 0) \
  G(0, ft128, tap, "gemm.hid.ft128.tap", 0) \
  G(0, ft128, prod, "gemm.hid.ft128.prod", 0) \
  G(1, ft128, tap, "gemm.out.ft128.tap", 0) \
  G(1, ft128, plain, "gemm.out.ft128.plain", 0) \
  G(1, ft128, anyw, "gemm.out.ft128.anyw", 0) \
  G(1, ft128, masked, "gemm.out.ft128.masked", 0) \
  G(1, ft128, masked_anyw, "gemm.out.ft128.masked_anyw", 0) \
  G(0, ft256, tap, "gemm.hid.ft256.tap", 0) \
  G(0, ft256, prod, "gemm.hid.ft256.prod", 0) \
  G(0, ft256, prod_nofix, "gemm.hid.ft256.prod_nofix", 0) \
  G(1, ft256, tap, "gemm.out.ft256.tap", 0) \
  G(1, ft256, plain, "gemm.out.ft256.plain", 0) \
  G(1, ft256, anyw, "gemm.out.ft256.anyw", 0) \
  G(1, ft256, masked, "gemm.out.ft256.masked", 0) \
  G(1, ft256, masked_anyw, "gemm.out.ft256.masked_anyw", 0) \
  G(1, ft256, fused, "gemm.out.ft256.fused", 0) \
  G(1, ft256, fused_masked, "gemm.out.ft256.fused_masked", 0) \
  G(1, ft256, fused_anyw, "gemm.out.ft256.fused_anyw", 0) \
  G(1, ft256, fused_masked_anyw, "gemm.out.ft256.fused_masked_anyw", 0) \
  G(1, ft256, fused_nofix, "gemm.out.ft256.fused_nofix", 0) \
  G(1, ft256, fused_masked_nofix, "gemm.out.ft256.fused_masked_nofix", 0) \
  G(0, ft320, tap, "gemm.hid.ft320.tap", 0) \
  G(0, ft320, prod, "gemm.hid.ft320.prod", 0) \
  G(0, ft320, prod_nofix, "gemm.hid.ft320.prod_nofix", 0) \
  G(1, ft320, tap, "gemm.out.ft320.tap", 0) \
  G(1, ft320, plain, "gemm.out.ft320.plain", 0) \
  G(1, ft320, anyw, "gemm.out.ft320.anyw", 0) \
  G(1, ft320, masked, "gemm.out.ft320.masked", 0) \
  G(1, ft320, masked_anyw, "gemm.out.ft320.masked_anyw", 0) \
  G(1, ft320, fused, "gemm.out.ft320.fused", 0) \
  G(1, ft320, fused_masked, "gemm.out.ft320.fused_masked", 0) \
  G(1, ft320, fused_anyw, "gemm.out.ft320.fused_anyw", 0) \
  G(1, ft320, fused_masked_anyw, "gemm.out.ft320.fused_masked_anyw", 0) \
  G(1, ft320, fused_nofix, "gemm.out.ft320.fused_nofix", 0) \
  G(1, ft320, fused_masked_nofix, "gemm.out.ft320.fused_masked_nofix", 0) \
  G(0, ft32bk64, tap, "gemm.hid.ft32.bk64.tap", 1) \
  G(0, ft32bk64, prod, "gemm.hid.ft32.bk64.prod", 1) \
  G(1, ft32bk64, tap, "gemm.out.ft32.bk64.tap", 1) \
  G(1, ft32bk64, plain, "gemm.out.ft32.bk64.plain", 1) \
  G(1, ft32bk64, anyw, "gemm.out.ft32.bk64.anyw", 1) \
  G(1, ft32bk64, masked, "gemm.out.ft32.bk64.masked", 1) \
  G(1, ft32bk64, masked_anyw, "gemm.out.ft32.bk64.masked_anyw", 1) \
  G(0, ft64bk64, tap, "gemm.hid.ft64.bk64.tap", 1) \
  G(0, ft64bk64, prod, "gemm.hid.ft64.bk64.prod", 1) \
  G(1, ft64bk64, tap, "gemm.out.ft64.bk64.tap", 1) \
  G(1, ft64bk64, plain, "gemm.out.ft64.bk64.plain", 1) \
  G(1, ft64bk64, anyw, "gemm.out.ft64.bk64.anyw", 1) \
  G(1, ft64bk64, masked, "gemm.out.ft64.bk64.masked", 1) \
  G(1, ft64bk64, masked_anyw, "gemm.out.ft64.bk64.masked_anyw", 1) \
  G(0, ft128bk64x6, prod, "gemm.hid.ft128.bk64x6.prod", 1) \
  G(1, ft128bk64x6, plain, "gemm.out.ft128.bk64x6.plain", 1) \
  G(1, ft128bk64x6, anyw, "gemm.out.ft128.bk64x6.anyw", 1) \
  G(1, ft128bk64x6, masked, "gemm.out.ft128.bk64x6.masked", 1) \
  G(1, ft128bk64x6, masked_anyw, "gemm.out.ft128.bk64x6.masked_anyw", 1) \
  G(1, ft128bk64x6, fused, "gemm.out.ft128.bk64x6.fused", 1) \
  G(1, ft128bk64x6, fused_masked, "gemm.out.ft128.bk64x6.fused_masked", 1) \
  G(1, ft128bk64x6, fused_anyw, "gemm.out.ft128.bk64x6.fused_anyw", 1) \
  G(1, ft128bk64x6, fused_masked_anyw, "gemm.out.ft128.bk64x6.fused_masked_anyw", 1)

// X(identifier, name, flags)   flags: 1 = the branch exists only in measurement builds (-DFDNN_ABLATION), 2 = runs at model load
#define FDNN_LAUNCH_NAMES(X) \
  X(unlisted, "unlisted", 0) /* a GEMM launch whose (shape, branch) the list above lacks: never, by launch_cfg's conditions */ \
  X(small_hid_nt32_tap, "small.hid.nt32.tap", 0) \
  X(small_hid_nt32_prod, "small.hid.nt32.prod", 0) \
  X(small_hid_nt64_tap, "small.hid.nt64.tap", 0) \
  X(small_hid_nt64_prod, "small.hid.nt64.prod", 0) \
  X(small_out_tap, "small.out.tap", 0) \
  X(small_out_masked, "small.out.masked", 0) \
  X(small_out_prod, "small.out.prod", 0) \
  X(chain_ft256_fix, "chain.ft256.fix", 0) \
  X(chain_ft256_nofix, "chain.ft256.nofix", 0) \
  X(chain_ft320_fix, "chain.ft320.fix", 0) \
  X(chain_ft320_nofix, "chain.ft320.nofix", 0) \
  X(pp_hid_fix, "pp.hid.fix", 0) \
  X(pp_hid_nofix, "pp.hid.nofix", 0) \
  X(ppo_out_fix, "ppo.out.fix", 0) \
  X(ppo_out_nofix, "ppo.out.nofix", 0) \
  X(l0_mfma_prod, "l0.mfma.prod", 0) \
  X(l0_mfma_tap, "l0.mfma.tap", 0) \
  X(l0_small_prod, "l0.small.prod", 0) \
  X(l0_small_tap, "l0.small.tap", 0) \
  X(l0_tile16_prod, "l0.tile16.prod", 0) \
  X(l0_tile16_tap, "l0.tile16.tap", 0) \
  X(l0_tile32_prod, "l0.tile32.prod", 0) \
  X(l0_tile32_tap, "l0.tile32.tap", 0) \
  X(l0_tile64_prod, "l0.tile64.prod", 0) \
  X(l0_tile64_tap, "l0.tile64.tap", 0) \
  X(l0_tile16_fma_prod, "l0.tile16.fma.prod", 1) \
  X(l0_tile16_fma_tap, "l0.tile16.fma.tap", 1) \
  X(l0_tile32_fma_prod, "l0.tile32.fma.prod", 1) \
  X(l0_tile32_fma_tap, "l0.tile32.fma.tap", 1) \
  X(l0_tile64_fma_prod, "l0.tile64.fma.prod", 1) \
  X(l0_tile64_fma_tap, "l0.tile64.fma.tap", 1) \
  X(l0_image_frames, "l0.image.frames", 0) \
  X(l0_image_weights, "l0.image.weights", 2) \
  X(l0_chain_jc12_tn64_prod, "l0.chain.jc12.tn64.prod", 0) \
  X(l0_chain_jc12_tn64_tap, "l0.chain.jc12.tn64.tap", 0) \
  X(l0_chain_jc12_tn128_prod, "l0.chain.jc12.tn128.prod", 0) \
  X(l0_chain_jc12_tn128_tap, "l0.chain.jc12.tn128.tap", 0) \
  X(l0_chain_jc16_tn64_prod, "l0.chain.jc16.tn64.prod", 0) \
  X(l0_chain_jc16_tn64_tap, "l0.chain.jc16.tn64.tap", 0) \
  X(l0_chain_jc16_tn128_prod, "l0.chain.jc16.tn128.prod", 0) \
  X(l0_chain_jc16_tn128_tap, "l0.chain.jc16.tn128.tap", 0) \
  X(l0_screen_f128, "l0.screen.f128", 0) \
  X(l0_screen_f64, "l0.screen.f64", 1) \
  X(l0_fix_tiles, "l0.fix.tiles", 0) \
  X(l0_digits, "l0.digits", 0) \
  X(l0_split_n64, "l0.split.n64", 0) \
  X(l0_split_n128, "l0.split.n128", 0) \
  X(l0_split_n128_probe, "l0.split.n128.probe", 0) \
  X(l0_fixlist_lpo8, "l0.fixlist.lpo8", 0) \
  X(l0_fixlist_lpo4, "l0.fixlist.lpo4", 0) \
  X(l0_fixlist_nb2_lpo8, "l0.fixlist.nb2.lpo8", 1) \
  X(l0_fixlist_nb5_lpo4, "l0.fixlist.nb5.lpo4", 1) \
  X(l0_fixlist_t512, "l0.fixlist.t512", 1) \
  X(norm_small, "norm.small", 0) \
  X(norm_rows, "norm.rows", 0) \
  X(maskpack_flat, "maskpack.flat", 0) \
  X(maskpack_rows, "maskpack.rows", 0) \
  X(maskunpack, "maskunpack", 0) \
  X(compact, "compact", 0) \
  X(xor80, "xor80", 0) \
  X(splice, "splice", 0) \
  X(fastdiv_check, "fastdiv_check", 2)

constexpr int kLaunchAblation = 1, kLaunchLoadTime = 2;

enum LaunchName : int {
#define FDNN_X(id, name, flags) kLn_##id,
  FDNN_LAUNCH_NAMES(FDNN_X)
#undef FDNN_X
#define FDNN_G(out, shape, branch, name, abl) kLn_gemm_##out##_##shape##_##branch,
  FDNN_GEMM_LAUNCH_NAMES(FDNN_G)
#undef FDNN_G
  kLaunchNameCount
};

struct LaunchNameInfo {
  const char *name;
  int flags;
};
extern const LaunchNameInfo kLaunchNames[kLaunchNameCount];  // fdnn_debug.cpp
extern std::atomic<int> g_launch_note_on;
extern std::atomic<unsigned long long> g_launch_count[kLaunchNameCount];

// every launch site calls this with the name of the branch it takes
inline void note_launch(int id) {
  if (g_launch_note_on.load(std::memory_order_relaxed)) g_launch_count[id].fetch_add(1, std::memory_order_relaxed);
}
// a launcher that starts two kernels names both under the one load
inline void note_launch(int id, int id2) {
  if (g_launch_note_on.load(std::memory_order_relaxed)) {
    g_launch_count[id].fetch_add(1, std::memory_order_relaxed);
    g_launch_count[id2].fetch_add(1, std::memory_order_relaxed);
  }
}
int gemm_launch_name(bool output, int shape, int branch);  // fdnn_debug.cpp; kLn_unlisted where the list lacks the combination

}  // namespace fdnn
