// fdnn_loglik.hip -- the dense output as DECODER SCORES: of every row of probabilities ln(p_i) - log_prior[i], floored,
// as fp32 or fp16 (fdnn_loglik.hpp: the logarithm, the score, the plan, the host restatement -- the arithmetic is the
// header's, called from here).
//
//   CalculateOutput (dnn.cc:428-454) hands every caller output_dim probabilities per frame; a hybrid decoder takes their
//   logarithm and subtracts the log priors on the host after 3.2 MB per 100 frames of the 8000-node net have crossed PCIe.
//   Here the device does both, and the scores -- which fit fp16 where probabilities do not -- can leave at half the bytes.
//
// loglik_rows_kernel<F16, VEC>: a workgroup of 256 threads takes rows_per_block rows (16, or 4 where that would leave the
// card short of workgroups: the plan) x (256 x cols) columns.  A thread owns `cols` consecutive columns, reads their priors
// ONCE into registers and walks down the rows, the loads of kRowsInFlight rows issued before the first value is used (the
// pass is bound by memory; the ~20 VALU instructions an element hide behind it).
//   * VEC (width % 4 == 0, both bases on a 16-byte boundary): cols = 4 (F32) or 8 (F16); 16-byte loads, 16-byte stores.
//     An F16 row of a width that is no multiple of 8 starts on an 8-byte boundary only: its stores go as two 8-byte halves,
//     and the thread that owns the row's last four columns has the first half alone.
//   * scalar access (any width, element alignment): cols = 1.
// loglik_entries_kernel<F16>: one (node, p) entry per lane; the prior is gathered (the L2 serves it), a node outside
// [0, width) gives a NaN and reads nothing.
//
// No atomics, no LDS, no device state that outlives a launch, no inline assembly.  Built WITHOUT a flush-to-zero or
// fast-math flag and with -ffp-contract=off (csrc/Makefile): the header's sequence is what runs.
#include "fdnn_device.hpp"
#include "fdnn_kernels.hpp"
#include "fdnn_launch.hpp"
#include "fdnn_loglik.hpp"

namespace fdnn {
namespace {

using namespace loglik;

LaunchCounts<3> g_loglik_launches;  // rows vector, rows scalar, entries
std::atomic<int> g_loglik_mode{0};  // fdnn_debug_set_loglik_kernel

// the hardware's fp32 -> fp16 conversion: round to nearest even, denormals kept (loglik::half_bits states it)
__device__ inline uint32_t half_of(float s) { return __builtin_bit_cast(uint16_t, static_cast<_Float16>(s)); }
__device__ inline uint32_t half2_of(float lo, float hi) { return half_of(lo) | (half_of(hi) << 16); }

template <bool F16, bool VEC>
__global__ __launch_bounds__(kThreads) void loglik_rows_kernel(const float *rows, int n, int rows_per_block, int width, const float *prior, float floor, void *out) {
  constexpr int COLS = VEC ? (F16 ? 8 : 4) : 1;
  constexpr int U = kRowsInFlight;
  const int c0 = (static_cast<int>(blockIdx.y) * kThreads + static_cast<int>(threadIdx.x)) * COLS;
  if (c0 >= width) return;
  const int r0 = static_cast<int>(blockIdx.x) * rows_per_block, rend = min(n, r0 + rows_per_block);
  const bool second = VEC && F16 && c0 + 8 <= width;  // (an F16 vector thread's columns 4 .. 7 are in the row)
  const bool pitch16 = (width & 7) == 0;              // (F16 vector rows start on a 16-byte boundary)

  float lp[COLS];
  if constexpr (VEC) {
    const float4 a = *reinterpret_cast<const float4 *>(prior + c0);
    lp[0] = a.x, lp[1] = a.y, lp[2] = a.z, lp[3] = a.w;
    if constexpr (F16) {
      float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (second) b = *reinterpret_cast<const float4 *>(prior + c0 + 4);
      lp[4] = b.x, lp[5] = b.y, lp[6] = b.z, lp[7] = b.w;
    }
  } else {
    lp[0] = prior[c0];
  }

  for (int r = r0; r < rend; r += U) {
    float v[U][COLS];
#pragma unroll
    for (int u = 0; u < U; ++u) {  // every load of the group is issued before the first value is used
      if (r + u >= rend) continue;
      const float *src = rows + static_cast<size_t>(r + u) * width + c0;
      if constexpr (VEC) {
        const float4 a = *reinterpret_cast<const float4 *>(src);
        v[u][0] = a.x, v[u][1] = a.y, v[u][2] = a.z, v[u][3] = a.w;
        if constexpr (F16) {
          float4 b = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
          if (second) b = *reinterpret_cast<const float4 *>(src + 4);
          v[u][4] = b.x, v[u][5] = b.y, v[u][6] = b.z, v[u][7] = b.w;
        }
      } else {
        v[u][0] = *src;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (r + u >= rend) continue;
      const size_t at = static_cast<size_t>(r + u) * width + c0;
      float s[COLS];
#pragma unroll
      for (int j = 0; j < COLS; ++j) s[j] = score(v[u][j], lp[j], floor);
      if constexpr (!F16) {
        float *dst = static_cast<float *>(out) + at;
        if constexpr (VEC)
          *reinterpret_cast<float4 *>(dst) = make_float4(s[0], s[1], s[2], s[3]);
        else
          *dst = s[0];
      } else {
        uint16_t *dst = static_cast<uint16_t *>(out) + at;
        if constexpr (VEC) {
          const uint2 lo = make_uint2(half2_of(s[0], s[1]), half2_of(s[2], s[3]));
          const uint2 hi = make_uint2(half2_of(s[4], s[5]), half2_of(s[6], s[7]));
          if (pitch16) {
            *reinterpret_cast<uint4 *>(dst) = make_uint4(lo.x, lo.y, hi.x, hi.y);
          } else {
            *reinterpret_cast<uint2 *>(dst) = lo;
            if (second) *reinterpret_cast<uint2 *>(dst + 4) = hi;
          }
        } else {
          *dst = static_cast<uint16_t>(half_of(s[0]));
        }
      }
    }
  }
}

template <bool F16>
__global__ __launch_bounds__(kThreads) void loglik_entries_kernel(const int32_t *nodes, const float *p, int count, int width, const float *prior, float floor, void *out) {
  const int j = static_cast<int>(blockIdx.x) * kThreads + static_cast<int>(threadIdx.x);
  if (j >= count) return;
  const int node = nodes[j];
  float s = float_of(0x7fc00000u);
  if (node >= 0 && node < width) s = score(p[j], prior[node], floor);
  if constexpr (F16)
    static_cast<uint16_t *>(out)[j] = static_cast<uint16_t>(half_of(s));
  else
    static_cast<float *>(out)[j] = s;
}

template <bool F16, bool VEC>
void launch_rows(const Plan &p, const float *rows, int n, int width, const float *prior, float floor, void *out, hipStream_t s) {
  const dim3 grid((n + p.rows_per_block - 1) / p.rows_per_block, p.grid_y);
  hipLaunchKernelGGL((loglik_rows_kernel<F16, VEC>), grid, dim3(kThreads), 0, s, rows, n, p.rows_per_block, width, prior, floor, out);
}

}  // namespace

void launch_loglik_rows(const float *d_rows, int n, int width, const float *d_log_prior, float floor, int type, void *d_out, hipStream_t s) {
  if (n <= 0 || width < 1 || width > kMaxWidth || (type != kF32 && type != kF16)) return;
  // (the form is chosen on the call's bases: width % 4 == 0 keeps every later launch's bases on the same boundary)
  const Plan p = loglik::plan(n, width, type, d_rows, d_out, g_loglik_mode.load(std::memory_order_relaxed));
  for (int r = 0; r < n; r += p.rows_per_launch) {
    const int cnt = std::min(p.rows_per_launch, n - r);
    const float *rows = d_rows + static_cast<size_t>(r) * width;
    void *out = static_cast<char *>(d_out) + static_cast<size_t>(r) * width * elem_bytes(type);
    g_loglik_launches.bump(p.form == kVector ? 0 : 1);
    if (p.form == kVector) {
      if (type == kF16) launch_rows<true, true>(p, rows, cnt, width, d_log_prior, floor, out, s);
      else launch_rows<false, true>(p, rows, cnt, width, d_log_prior, floor, out, s);
    } else {
      if (type == kF16) launch_rows<true, false>(p, rows, cnt, width, d_log_prior, floor, out, s);
      else launch_rows<false, false>(p, rows, cnt, width, d_log_prior, floor, out, s);
    }
  }
}

void launch_loglik_entries(const int32_t *d_nodes, const float *d_p, long long count, int width, const float *d_log_prior, float floor, int type, void *d_out, hipStream_t s) {
  if (count <= 0 || width < 1 || width > kMaxWidth || (type != kF32 && type != kF16)) return;
  for (long long at = 0; at < count; at += kMaxEntriesPerLaunch) {
    const int cnt = static_cast<int>(std::min<long long>(kMaxEntriesPerLaunch, count - at));
    void *out = static_cast<char *>(d_out) + static_cast<size_t>(at) * elem_bytes(type);
    g_loglik_launches.bump(2);
    const dim3 grid((cnt + kThreads - 1) / kThreads);
    if (type == kF16)
      hipLaunchKernelGGL(loglik_entries_kernel<true>, grid, dim3(kThreads), 0, s, d_nodes + at, d_p + at, cnt, width, d_log_prior, floor, out);
    else
      hipLaunchKernelGGL(loglik_entries_kernel<false>, grid, dim3(kThreads), 0, s, d_nodes + at, d_p + at, cnt, width, d_log_prior, floor, out);
  }
}

void loglik_launch_counts(unsigned long long out[3]) { g_loglik_launches.read(out); }
int loglik_kernel_mode() { return g_loglik_mode.load(std::memory_order_relaxed); }
void loglik_kernel_mode(int mode) { g_loglik_mode.store(mode, std::memory_order_relaxed); }

}  // namespace fdnn
