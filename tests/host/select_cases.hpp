// select_cases.hpp -- the switch settings and the frame range that the host checks of the selection sweep: select_check.cpp
// records and reproduces the choices over them, ctx_layout_check.cpp holds the context's buffer sizes against the same choices.
#pragma once
#include "fdnn_select.hpp"

namespace select_cases {

struct Setting {
  const char *name;
  int chain_mode, chain_min, pp_mode, pp_min, ppo_mode;  // fdnn_debug_set_chain / _pp / _ppo
  bool fuse_off;                                         // FDNN_FUSE_NORM=0
  bool taps, byte_mask, bit_mask;                        // what the call carries
};
const Setting kSettings[] = {
    {"defaults", -1, 0, -1, 0, -1, false, false, false, false},
    {"chain0", 0, 0, -1, 0, -1, false, false, false, false},
    {"chain1", 1, 0, -1, 0, -1, false, false, false, false},
    {"chain1.min5000", 1, 5000, -1, 0, -1, false, false, false, false},
    {"pp0", -1, 0, 0, 0, -1, false, false, false, false},
    {"pp1", -1, 0, 1, 0, -1, false, false, false, false},
    {"pp1.min3000", -1, 0, 1, 3000, -1, false, false, false, false},
    {"ppo0", -1, 0, -1, 0, 0, false, false, false, false},
    {"ppo1", -1, 0, -1, 0, 1, false, false, false, false},
    {"fuse_off", -1, 0, -1, 0, -1, true, false, false, false},
    {"taps", -1, 0, -1, 0, -1, false, true, false, false},
    {"byte_mask", -1, 0, -1, 0, -1, false, false, true, false},
    {"bit_mask", -1, 0, -1, 0, -1, false, false, false, true},
};
constexpr int kMaxFrames = 70000;  // every frame count 1 .. kMaxFrames is visited

// the process's switches as the setting leaves them
inline fdnn::sel::Tuning tuning_of(const Setting &s) {
  fdnn::sel::Tuning t;
  t.chain_mode = s.chain_mode;
  t.chain_min = s.chain_min;
  t.pp_mode = s.pp_mode;
  t.pp_min = s.pp_min;
  t.ppo_mode = s.ppo_mode;
  if (s.fuse_off) t.fuse_norm = 0;
  return t;
}

}  // namespace select_cases
