// fdnn_select.cpp -- the process's switches (fdnn_select.hpp: Tuning), read from the environment once, at first use.
#include "fdnn_select.hpp"

#include <cstdlib>

#include "fdnn_kernels.hpp"  // FDNN_TUNE_ENV: null outside measurement builds

namespace fdnn::sel {
namespace {

void read_int(const char *e, int *v) {
  if (e) *v = std::atoi(e);
}

Tuning from_environment() {
  Tuning t;
  read_int(std::getenv("FDNN_CHAIN"), &t.chain_env);
  read_int(std::getenv("FDNN_CHAIN_MIN"), &t.chain_min_env);
  read_int(std::getenv("FDNN_PP"), &t.pp_env);
  read_int(std::getenv("FDNN_PP_MIN"), &t.pp_min_env);
  read_int(std::getenv("FDNN_PP_ONLY"), &t.pp_only);
  read_int(std::getenv("FDNN_PPO"), &t.ppo_env);
  if (const char *e = std::getenv("FDNN_FUSE_NORM")) t.fuse_norm = std::atoi(e) != 0 ? 1 : 0;
  read_int(std::getenv("FDNN_GEMM_DEBUG"), &t.gemm_debug);
  if (const char *e = std::getenv("FDNN_L0_TN")) t.l0_chain_tn = std::atoi(e) == 128 ? 128 : 64;
  if (const char *e = std::getenv("FDNN_CHUNK_FRAMES")) t.chunk_set = true, t.chunk_frames = std::atoi(e);
  read_int(FDNN_TUNE_ENV("FDNN_FRAME_TILE"), &t.frame_tile);
  read_int(FDNN_TUNE_ENV("FDNN_NODE_TILE"), &t.node_tile);
  read_int(FDNN_TUNE_ENV("FDNN_SMALL_MAX"), &t.small_max);
  read_int(FDNN_TUNE_ENV("FDNN_SMALL_WM"), &t.small_wm);
  read_int(FDNN_TUNE_ENV("FDNN_SMALL_NTM"), &t.small_ntm);
  read_int(FDNN_TUNE_ENV("FDNN_CHAIN_TILE"), &t.chain_tile);
  if (const char *e = FDNN_TUNE_ENV("FDNN_SMALL_BK")) t.small_bk64 = std::atoi(e) != 128;
  read_int(FDNN_TUNE_ENV("FDNN_FUSE_STAGGER"), &t.fuse_stagger);
  t.l0_fma_valu = FDNN_TUNE_ENV("FDNN_L0_FMA_VALU") != nullptr;
  t.l0_no_screen = FDNN_TUNE_ENV("FDNN_L0_NO_SCREEN") != nullptr;
  t.l0_classic = FDNN_TUNE_ENV("FDNN_L0_CLASSIC") != nullptr;
  t.l0_no_split = FDNN_TUNE_ENV("FDNN_L0_NO_SPLIT") != nullptr;
  read_int(FDNN_TUNE_ENV("FDNN_L0_SMALL_MAX"), &t.l0_small_max);
  read_int(FDNN_TUNE_ENV("FDNN_L0_SPLIT_MIN"), &t.l0_split_min);
  read_int(FDNN_TUNE_ENV("FDNN_L0_T64_BK"), &t.l0_t64_bk);
  if (const char *e = FDNN_TUNE_ENV("FDNN_L0_SCREEN_WFR")) t.l0_screen_wfr = std::atoi(e) == 2 ? 2 : 4;
  read_int(FDNN_TUNE_ENV("FDNN_L0S_WN"), &t.l0s_wn);
  read_int(FDNN_TUNE_ENV("FDNN_L0_FIX_NB"), &t.l0_fix_nb);
  read_int(FDNN_TUNE_ENV("FDNN_L0_FIX_T"), &t.l0_fix_t);
  read_int(FDNN_TUNE_ENV("FDNN_L0_FIX_LPO"), &t.l0_fix_lpo);
  return t;
}

}  // namespace

Tuning &tuning() {
  static Tuning t = from_environment();
  return t;
}

}  // namespace fdnn::sel
