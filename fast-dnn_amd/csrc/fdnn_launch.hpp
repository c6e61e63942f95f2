// fdnn_launch.hpp -- host-side helpers the lazy launchers share (fdnn_lists.hip, fdnn_set.hip, fdnn_sets.hip,
// fdnn_lists_union.hip): their launch counters and the choice of a score kernel's <FIX, FAST> instance.
#pragma once
#include <atomic>
#include <type_traits>

namespace fdnn {

// N launch counts behind one fdnn_debug_*_launches call: bumped where a launch is enqueued, read as a snapshot.
template <int N>
struct LaunchCounts {
  std::atomic<unsigned long long> v[N];
  void bump(int i) { v[i].fetch_add(1, std::memory_order_relaxed); }
  void read(unsigned long long out[N]) const {
    for (int i = 0; i < N; ++i) out[i] = v[i].load(std::memory_order_relaxed);
  }
};

// f(FIX, FAST) with the two as std::bool_constant values: the instance of a score kernel template that a layer takes.
// FIX: the layer has saturating pairs (both halves of the per-node index are there); FAST: validated 3-operation division.
template <class F>
void with_fix_fast(bool fix, bool fast, F &&f) {
  if (fix && fast)
    f(std::true_type{}, std::true_type{});
  else if (fix)
    f(std::true_type{}, std::false_type{});
  else if (fast)
    f(std::false_type{}, std::true_type{});
  else
    f(std::false_type{}, std::false_type{});
}

}  // namespace fdnn
