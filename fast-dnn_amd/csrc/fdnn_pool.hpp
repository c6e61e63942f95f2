// fdnn_pool.hpp -- the HIP-free half of the dense output POOLED over a node -> class map (fdnn_pool.hip): the map and its
// CSR, the order of the additions, the launch plan of a (rows x width, C classes) pooling and a plain host restatement of it.
// tests/host/pool_check.cpp builds this header alone, under the sanitizers.
//
// The pooling extends CalculateOutput (src/cpp/dnn.cc:428-454): of a row p[0 .. W) of probabilities the sum over every class
// of output nodes.  A map class_of[0 .. W) puts node i into class class_of[i] in [0, C) or, with -1, into none; the members
// of class c in ascending node order are m_0 < m_1 < ... < m_{L-1}, and
//
//   s_j = +0.0f;  for t = j, j + 16, j + 32, ... (t < L):  s_j = s_j + p[m_t]          j = 0 .. kPoolLanes - 1
//   q_c = (((s_0+s_1)+(s_2+s_3)) + ((s_4+s_5)+(s_6+s_7))) + (((s_8+s_9)+(s_10+s_11)) + ((s_12+s_13)+(s_14+s_15)))
//
// every + one fp32 addition, round to nearest even, denormals kept (no flush-to-zero, no fast-math: neither in the kernel
// file nor where this header is built).  An empty class gives +0.0f; a singleton its value's own bits (-0 becomes +0).
// q_c depends on the row and the map alone: not on the row's position, the batch, the entry point or the kernel form.
// Sixteen partials = one DPP row of a gfx950 wave; the tree is the xor-1/2/4/8 butterfly read at lane 0.  FROZEN: results
// depend on kPoolLanes.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace fdnn {
namespace pool {

constexpr int kPoolLanes = 16;               // partial sums of a class: one 16-lane group of a wave
constexpr int kPoolResidentWidth = 16384;    // rows up to this width are held in LDS (64 KiB)
constexpr int kThreads = 256;                // one workgroup per row ...
constexpr int kGroups = kThreads / kPoolLanes;  // ... whose 16-lane groups take a class at a time
constexpr int kMaxWidth = 1 << 19;           // the loader's widest output layer
constexpr int kMaxRowsPerLaunch = 1 << 20;   // a longer call goes as several launches
constexpr int kLdsLimit = 160 * 1024;        // LDS of a gfx950 CU
static_assert(kPoolLanes == 16, "the tree below and the kernel's four DPP steps are written for sixteen partials");
static_assert((kPoolResidentWidth + 4) * 4 <= kLdsLimit, "a resident row fits the CU's LDS");

// ---------------------------------------------------------------- the map
// 0 when class_of[0 .. width) is a map onto n_classes classes (1 <= C <= W, every entry -1 or in [0, C)), else 1 + the index
// of the first bad entry, or -1 for bad counts / a null map
inline long long check_map(const int32_t *class_of, int width, int n_classes) {
  if (!class_of || width < 1 || width > kMaxWidth || n_classes < 1 || n_classes > width) return -1;
  for (int i = 0; i < width; ++i)
    if (class_of[i] < -1 || class_of[i] >= n_classes) return 1 + static_cast<long long>(i);
  return 0;
}

// class_ptr [C + 1], member [nnz]: the mapped nodes sorted by class, then by node (a counting sort over a checked map)
struct Csr {
  std::vector<int32_t> class_ptr, member;
};
inline Csr build_csr(const int32_t *class_of, int width, int n_classes) {
  Csr c;
  c.class_ptr.assign(static_cast<size_t>(n_classes) + 1, 0);
  for (int i = 0; i < width; ++i)
    if (class_of[i] >= 0) ++c.class_ptr[static_cast<size_t>(class_of[i]) + 1];
  for (int k = 0; k < n_classes; ++k) c.class_ptr[static_cast<size_t>(k) + 1] += c.class_ptr[static_cast<size_t>(k)];
  c.member.resize(static_cast<size_t>(c.class_ptr[static_cast<size_t>(n_classes)]));
  std::vector<int32_t> at(c.class_ptr.begin(), c.class_ptr.end() - 1);
  for (int i = 0; i < width; ++i)
    if (class_of[i] >= 0) c.member[static_cast<size_t>(at[static_cast<size_t>(class_of[i])]++)] = i;
  return c;
}

// ---------------------------------------------------------------- the sum, over bit patterns
inline uint32_t add_bits(uint32_t a, uint32_t b) {
  float x, y;
  std::memcpy(&x, &a, 4), std::memcpy(&y, &b, 4);
  volatile float z = x + y;  // (one rounding to fp32, whatever the host's evaluation width)
  const float w = z;
  uint32_t r;
  std::memcpy(&r, &w, 4);
  return r;
}

// One class of one row: members member[0 .. len) of row[]
inline uint32_t ref_class(const uint32_t *row, const int32_t *member, int len) {
  uint32_t s[kPoolLanes];
  for (int j = 0; j < kPoolLanes; ++j) {
    s[j] = 0u;  // +0.0f
    for (int t = j; t < len; t += kPoolLanes) s[j] = add_bits(s[j], row[member[t]]);
  }
  for (int d = 1; d < kPoolLanes; d <<= 1)  // (s_0+s_1), ((s_0+s_1)+(s_2+s_3)), ...: the butterfly as lane 0 sees it
    for (int j = 0; j < kPoolLanes; j += 2 * d) s[j] = add_bits(s[j], s[j + d]);
  return s[0];
}

// The pooling in plain C++: rows [n][width] as bit patterns, results [n][n_classes]
inline void ref(const uint32_t *rows, int n, int width, const int32_t *class_ptr, const int32_t *member, int n_classes, uint32_t *out) {
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n_classes; ++c)
      out[static_cast<size_t>(r) * n_classes + c] =
          ref_class(rows + static_cast<size_t>(r) * width, member + class_ptr[c], class_ptr[c + 1] - class_ptr[c]);
}

// Additions a member of a class of len nodes passes through at most (the first, 0 + x, is exact): the derived bound is
// |q_c - sum| <= d u / (1 - d u) * sum |p_i|, u = 2^-24
inline int depth(int len) { return (len + kPoolLanes - 1) / kPoolLanes + 4; }

// ---------------------------------------------------------------- the launch plan
enum Form { kResident = 0, kStreaming = 1 };

// mode (fdnn_debug_set_pool_kernel): 0 the rule -- resident up to kPoolResidentWidth --, 1 resident where the width allows,
// 2 always streaming
inline Form form_for(int width, int mode) { return (mode == 2 || width > kPoolResidentWidth) ? kStreaming : kResident; }

struct Plan {
  Form form;
  int rows_per_launch;  // workgroups of a launch: one per row
  int launches;
  int lds_bytes;        // dynamic LDS of a workgroup
};

// The resident row sits in LDS shifted by its misalignment (0 .. 3 words), so that a 16-byte global load lands as a 16-byte
// LDS store: width + 4 words cover every shift.
inline Plan plan(int n, int width, int mode) {
  Plan p{form_for(width, mode), 0, 0, 0};
  p.rows_per_launch = std::min(std::max(n, 0), kMaxRowsPerLaunch);
  p.launches = p.rows_per_launch ? (n + p.rows_per_launch - 1) / p.rows_per_launch : 0;
  p.lds_bytes = p.form == kResident ? 4 * (width + 4) : 0;
  return p;
}

}  // namespace pool
}  // namespace fdnn
