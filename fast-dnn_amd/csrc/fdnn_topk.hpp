// fdnn_topk.hpp -- the HIP-free half of the dense output with a TOP-K RETURN (fdnn_topk.hip): the order on fp32 values,
// the launch plan of a (rows x width, k) selection and a plain host restatement of it.  tests/host/topk_check.cpp builds
// this header alone, under the sanitizers.
//
// The selection extends CalculateOutput (src/cpp/dnn.cc:428-454): of a row p[0 .. W) of probabilities the k first-ranked
// nodes and their values, in rank order.  Node i ranks before node j when key(p[i]) > key(p[j]), or the keys are equal
// and i < j.  The values returned are the row's own 32 bits.  The top k is a prefix of the top k + 1.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define FDNN_TOPK_HD __host__ __device__
#else
#define FDNN_TOPK_HD
#endif

namespace fdnn {
namespace topk {

constexpr int kTopkMaxK = 256;               // one candidate per thread of the workgroup
constexpr int kTopkResidentWidth = 16384;    // rows up to this width are held in LDS as keys (64 KiB)
constexpr int kThreads = 256;                // one workgroup per row
constexpr int kDigitBits = 8, kBins = 1 << kDigitBits;  // radix select: four passes over the 32-bit key
constexpr int kHistCopies = 4;               // every bin kept per (lane & 3): a quarter of the same-address LDS atomics
constexpr int kMaxRowsPerLaunch = 1 << 20;   // a longer call goes as several launches
constexpr int kLdsLimit = 160 * 1024;        // LDS of a gfx950 CU

// LDS of a workgroup, in 32-bit words: the digit histogram (after the passes: the sorted pairs), the candidates as
// 64-bit (key, ~node) words, scan scratch, and in the resident form the row's keys, shifted by the row's misalignment so
// that 16-byte global loads land as 16-byte LDS stores.
constexpr int kHistWords = kBins * kHistCopies;
constexpr int kCandWords = 2 * kTopkMaxK;
constexpr int kMiscWords = 16;
constexpr int kKeysAt = kHistWords + kCandWords + kMiscWords;
static_assert(kHistWords >= 2 * kTopkMaxK, "the sorted pairs reuse the histogram");
static_assert(kThreads == kBins && kThreads == kTopkMaxK, "a thread per bin of the scan and per candidate of the sort");
static_assert(kKeysAt % 4 == 0, "the staged keys start 16-byte aligned");

// The usual total order on floats as an unsigned number: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN
FDNN_TOPK_HD inline uint32_t key(uint32_t u) { return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u); }
FDNN_TOPK_HD inline uint32_t unkey(uint32_t k) { return k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu); }
// Does (key_i, node i) rank before (key_j, node j)?
FDNN_TOPK_HD inline bool ranks_before(uint32_t key_i, int i, uint32_t key_j, int j) { return key_i > key_j || (key_i == key_j && i < j); }
// Both as one comparison: the larger word ranks first (nodes of a row are distinct, so words are)
FDNN_TOPK_HD inline uint64_t pair_word(uint32_t k, int node) { return (static_cast<uint64_t>(k) << 32) | static_cast<uint32_t>(~node); }

inline bool args_ok(int width, int k) { return width >= 1 && k >= 1 && k <= std::min(width, kTopkMaxK); }

enum Form { kResident = 0, kStreaming = 1 };

// mode (fdnn_debug_set_topk_kernel): 0 the rule -- resident up to kTopkResidentWidth --, 1 resident where the width
// allows, 2 always streaming
inline Form form_for(int width, int mode) { return (mode == 2 || width > kTopkResidentWidth) ? kStreaming : kResident; }

struct Plan {
  Form form;
  int rows_per_launch;  // workgroups of a launch: one per row
  int launches;
  int lds_bytes;        // dynamic LDS of a workgroup
};

inline Plan plan(int n, int width, int mode) {
  Plan p{form_for(width, mode), 0, 0, 0};
  p.rows_per_launch = std::min(std::max(n, 0), kMaxRowsPerLaunch);
  p.launches = p.rows_per_launch ? (n + p.rows_per_launch - 1) / p.rows_per_launch : 0;
  p.lds_bytes = 4 * (kKeysAt + (p.form == kResident ? width + 4 : 0));
  return p;
}

// The selection in plain C++: rows [n][width] as bit patterns, results [n][k].  A partial sort by the rank comparison.
inline void ref(const uint32_t *rows, int n, int width, int k, int32_t *nodes, uint32_t *vals) {
  std::vector<int32_t> idx(static_cast<size_t>(width));
  for (int r = 0; r < n; ++r) {
    const uint32_t *row = rows + static_cast<size_t>(r) * width;
    for (int i = 0; i < width; ++i) idx[static_cast<size_t>(i)] = i;
    std::partial_sort(idx.begin(), idx.begin() + k, idx.end(), [row](int32_t a, int32_t b) { return ranks_before(key(row[a]), a, key(row[b]), b); });
    for (int j = 0; j < k; ++j) {
      nodes[static_cast<size_t>(r) * k + j] = idx[static_cast<size_t>(j)];
      vals[static_cast<size_t>(r) * k + j] = row[idx[static_cast<size_t>(j)]];
    }
  }
}

}  // namespace topk
}  // namespace fdnn
