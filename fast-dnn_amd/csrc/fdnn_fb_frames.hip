// fdnn_fb_frames.hip -- ALIGNMENT GRAPHS, SUMMED, FRAME BY FRAME: a graph's likelihood at every frame of a segment, with a
// start that may be free and a row carried from one call to the next (fdnn_fb_frames.hpp: the contract, the plan and the host
// restatement; the arithmetic is fdnn_fb.hpp's accumulate, ladd and the total's order, called from here).
//
//   The caller with a keyword graph against a filler, or doing end-pointing, had one fdnn_calculate_fb call per prefix or
//   the lazy sets over PCIe and the host's forward recursion.
//
// TWO launches per sweep; the per-frame total does not ride on the serial sweep.
//
// 1. The forward sweep, the sibling's row loop (fdnn_fb.hip) without a total.
//    frames_wave_kernel<K, TYPE, FREE>: one wave per segment, S <= 64 K <= kWaveStates.  Lane l owns states l, l + 64, .. and
//    keeps their start_of values in registers for the free-start term; d as two LDS rows; the loads of the next 16 / K rows
//    in flight while the current ones are stepped, their emissions waiting in an LDS ring; the arc offsets, and the arc table
//    where it has at most kArcLdsArcs arcs, staged in LDS once; no workgroup barrier.
//    frames_wg_kernel<TYPE, FREE>: 256 threads per segment, any S <= kMaxStates; one barrier per frame.
//    With alpha_in the first row of d is loaded from it and frame 0 takes the ordinary step; else frame 0 is the start row.
//    Every alpha[t][.] goes to the call's scratch lattice, coalesced, and nothing waits for those stores; the last row goes
//    to alpha_out.
// 2. frames_total_kernel: parallel over (segment, frame).  One wave per lattice row, four rows per workgroup.  Lane l owns
//    partials l, l + 64, l + 128, l + 192 and walks each partial's states in ascending order -- 64 consecutive floats a load
//    across the wave --, so the tree's steps 128 and 64 stay inside the lane and 32 .. 1 go over the lanes: the tree of
//    fb_wave_kernel's epilogue, for any S.
// Every arc index is bounded by the HOST table's counts (Launch::arc0 / n_arcs), whatever the device copies hold.
//
// No atomics, no inline assembly, no device state that outlives a launch.  Built WITHOUT a flush-to-zero or fast-math flag
// and with -ffp-contract=off (csrc/Makefile): the header's sequence is what runs.
#include "fdnn_device.hpp"
#include "fdnn_kernels.hpp"
#include "fdnn_launch.hpp"
#include "fdnn_fb_frames.hpp"

namespace fdnn {
namespace {

using namespace fb;
using fb_frames::kRowsPerGroup;
using fb_frames::RowLaunch;

LaunchCounts<3> g_frames_launches;  // sweep wave, sweep workgroup, row totals

struct Args {
  const float *rows;
  const int32_t *col, *node;  // node: null without a handle
  const float *prior;         // the handle's log priors [width]
  int width;
  float floor;
  const int32_t *ptr, *src;
  const float *lp;
  const float *start_lp, *final_lp;  // null = state 0 / state S - 1
  const float *alpha_in;             // [states of the call] or null
  float *alpha_out;                  // the same, or null
  float *lat;                        // the lattice
  float *frame_total;
};

struct State {
  int col;
  float prior;
};

template <int TYPE>
__device__ inline State load_state(const Args &a, int at, bool in, int ld) {
  State st{-1, 0.0f};
  if (!in) return st;
  const int c = a.col[at];
  st.col = (c >= 0 && c < ld) ? c : -1;
  if constexpr (TYPE != kScores) {
    const int nd = a.node[at];
    if (nd >= 0 && nd < a.width) st.prior = a.prior[nd];
    else st.col = -1;
  }
  return st;
}

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the wave's earlier LDS writes before its later LDS reads: the hardware serves one wave's LDS accesses in order, the fences
// keep the compiler from moving them
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A slot's value of row t; col is -1 where the slot has no state or its column or node is out of range: the load goes to
// column 0 of the row (inside it: ld >= 1) and the value is made a NaN by its bits, as in the sibling
__device__ __forceinline__ float row_value(const float *rows, int t, int ld, int col) {
  const int bad = col >> 31;  // 0 or all ones
  const float v = rows[static_cast<size_t>(t) * static_cast<size_t>(ld) + static_cast<size_t>(col & ~bad)];
  return float_of(bits_of(v) | (static_cast<uint32_t>(bad) & kQuietNaN));
}

// The wave form's frames first .. T - 1, stepped from the row in cur.  Frames go in groups of D = frames_in_flight(K): the
// group's emissions are put into the LDS ring from the values that came in during the group before, the loads of the NEXT
// group are issued, and then the group's frames are stepped.
template <int K, int TYPE, bool FREE, bool STAGED>
__device__ __forceinline__ void wave_frames(const Args &a, const float *rows, size_t out, int first, int T, int S, int ld, int lane, int arc0,
                                            const int (&col)[K], const float (&prior)[K], const float (&start)[K], float *cur, float *nxt, float *em,
                                            const int *abeg, const float *alp, const uint16_t *asrc, float **last) {
  constexpr int D = frames_in_flight(K);
  const float ninf = float_of(kMinusInf), nan = float_of(kQuietNaN);
  float v[D][K];
#pragma unroll
  for (int u = 0; u < D; ++u)
#pragma unroll
    for (int k = 0; k < K; ++k) v[u][k] = first + u < T ? row_value(rows, first + u, ld, col[k]) : nan;  // (uniform)
  for (int u0 = first; u0 < T; u0 += D) {
#pragma unroll
    for (int u = 0; u < D; ++u)
#pragma unroll
      for (int k = 0; k < K; ++k) em[(u * K + k) * kWaveLanes + lane] = align::emission(v[u][k], prior[k], a.floor, TYPE);  // (a lane's own states)
#pragma unroll
    for (int u = 0; u < D; ++u)
      if (u0 + D + u < T) {  // (uniform) in flight during the steps below
#pragma unroll
        for (int k = 0; k < K; ++k) v[u][k] = row_value(rows, u0 + D + u, ld, col[k]);
      }
#pragma unroll
    for (int u = 0; u < D; ++u) {
      if (u0 + u < T) {  // (uniform)
        const int t = u0 + u;
        const float *e = em + u * K * kWaveLanes;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int j = lane + k * kWaveLanes;
          if (j < S) {
            const int a0 = abeg[j], a1 = abeg[j + 1];
            float acc = ninf;
            for (int i = a0; i < a1; ++i) {
              int src;
              float lp;
              if constexpr (STAGED) {
                src = asrc[i], lp = alp[i];
              } else {
                src = a.src[arc0 + i], lp = a.lp[arc0 + i];
              }
              acc = accumulate(acc, static_cast<unsigned>(src) < static_cast<unsigned>(S) ? cur[src] : nan, lp);
            }
            if constexpr (FREE) acc = ladd(acc, start[k]);  // the start term, last
            const float val = acc + e[j];
            nxt[j] = val;
            a.lat[out + static_cast<size_t>(t) * static_cast<size_t>(S) + static_cast<size_t>(j)] = val;
          }
        }
        wave_sync();
        float *sw = cur;
        cur = nxt, nxt = sw;
      }
    }
  }
  *last = cur;
}

template <int K, int TYPE, bool FREE>
__global__ __launch_bounds__(kWaveLanes) void frames_wave_kernel(const Launch L, const Args a) {
  extern __shared__ uint32_t lds32[];
  const int seg = static_cast<int>(blockIdx.x), lane = static_cast<int>(threadIdx.x);
  const int T = L.T[seg], S = L.S[seg], ld = L.ld[seg], s0 = L.state0[seg], arc0 = L.arc0[seg], n_arcs = L.n_arcs[seg];
  const float *rows = a.rows + L.row_off[seg];
  const size_t out = static_cast<size_t>(L.out_off[seg]);
  float *cur = reinterpret_cast<float *>(lds32), *nxt = cur + L.d_floats, *em = nxt + L.d_floats;
  int *abeg = reinterpret_cast<int *>(em + kEmissionRing);
  float *alp = reinterpret_cast<float *>(abeg + L.d_floats + 64);
  uint16_t *asrc = reinterpret_cast<uint16_t *>(alp + L.arc_cap);
  const bool staged = n_arcs <= L.arc_cap;  // (the plan's rule: arc_cap is the largest staged count of the launch, at most kArcLdsArcs)
  const bool carried = a.alpha_in != nullptr;

  // the arc offsets, local to the segment and inside the host table's count whatever the device copy holds
  for (int j = lane; j <= S; j += kWaveLanes) abeg[j] = clampi(a.ptr[s0 + j] - arc0, 0, n_arcs);
  if (staged)
    for (int i = lane; i < n_arcs; i += kWaveLanes) {
      const int src = a.src[arc0 + i];
      alp[i] = a.lp[arc0 + i];
      asrc[i] = static_cast<unsigned>(src) < static_cast<unsigned>(S) ? static_cast<uint16_t>(src) : align_graph::kNoSource;
    }

  // slot k of a lane is state lane + 64 k (64 K >= the launch's largest graph, so d's rows hold every slot); the slots past S
  // have column -1 and hold NaNs nothing reads.  The first row of d: alpha_in, or the start row, which is frame 0's alpha
  int col[K];
  float prior[K], start[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int j = lane + k * kWaveLanes;
    const State st = load_state<TYPE>(a, s0 + j, j < S, ld);
    col[k] = st.col, prior[k] = st.prior;
    start[k] = j < S ? start_of(a.start_lp ? a.start_lp + s0 : nullptr, j) : float_of(kMinusInf);
    if (carried) {
      cur[j] = j < S ? a.alpha_in[s0 + j] : float_of(kQuietNaN);
    } else {
      const float val = start[k] + align::emission(row_value(rows, 0, ld, col[k]), prior[k], a.floor, TYPE);
      cur[j] = val;
      if (j < S) a.lat[out + static_cast<size_t>(j)] = val;
    }
  }
  wave_sync();
  float *last = cur;
  const int first = carried ? 0 : 1;
  if (staged) wave_frames<K, TYPE, FREE, true>(a, rows, out, first, T, S, ld, lane, arc0, col, prior, start, cur, nxt, em, abeg, alp, asrc, &last);
  else wave_frames<K, TYPE, FREE, false>(a, rows, out, first, T, S, ld, lane, arc0, col, prior, start, cur, nxt, em, abeg, alp, asrc, &last);
  if (a.alpha_out)
    for (int j = lane; j < S; j += kWaveLanes) a.alpha_out[s0 + j] = last[j];
}

template <int TYPE, bool FREE>
__global__ __launch_bounds__(kWgThreads) void frames_wg_kernel(const Launch L, const Args a) {
  extern __shared__ uint32_t lds32[];
  const int seg = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x);
  const int T = L.T[seg], S = L.S[seg], ld = L.ld[seg], s0 = L.state0[seg], arc0 = L.arc0[seg], n_arcs = L.n_arcs[seg];
  const float *rows = a.rows + L.row_off[seg];
  const size_t out = static_cast<size_t>(L.out_off[seg]);
  float *cur = reinterpret_cast<float *>(lds32), *nxt = cur + L.d_floats;
  const float ninf = float_of(kMinusInf), nan = float_of(kQuietNaN);
  const float *start_lp = a.start_lp ? a.start_lp + s0 : nullptr;
  const bool carried = a.alpha_in != nullptr;

  if (carried) {
    for (int j = tid; j < S; j += kWgThreads) cur[j] = a.alpha_in[s0 + j];
    __syncthreads();
  }
  for (int t = 0; t < T; ++t) {
    for (int j = tid; j < S; j += kWgThreads) {
      const State st = load_state<TYPE>(a, s0 + j, true, ld);
      const float v = st.col >= 0 ? rows[static_cast<size_t>(t) * static_cast<size_t>(ld) + static_cast<size_t>(st.col)] : nan;
      const float e = align::emission(v, st.prior, a.floor, TYPE);  // (does not depend on d)
      float acc;
      if (t == 0 && !carried) {
        acc = start_of(start_lp, j);
      } else {
        const int a0 = clampi(a.ptr[s0 + j] - arc0, 0, n_arcs), a1 = clampi(a.ptr[s0 + j + 1] - arc0, a0, n_arcs);
        acc = ninf;
        for (int i = a0; i < a1; ++i) {
          const int src = a.src[arc0 + i];
          acc = accumulate(acc, static_cast<unsigned>(src) < static_cast<unsigned>(S) ? cur[src] : nan, a.lp[arc0 + i]);
        }
        if constexpr (FREE) acc = ladd(acc, start_of(start_lp, j));  // the start term, last
      }
      const float val = acc + e;
      nxt[j] = val;
      a.lat[out + static_cast<size_t>(t) * static_cast<size_t>(S) + static_cast<size_t>(j)] = val;
    }
    __syncthreads();
    float *sw = cur;
    cur = nxt, nxt = sw;
  }
  if (a.alpha_out)
    for (int j = tid; j < S; j += kWgThreads) a.alpha_out[s0 + j] = cur[j];
}

// One wave per lattice row: blockIdx.y is the launch's segment, row blockIdx.x * kRowsPerGroup + the wave's index.  No
// barrier, so a wave past the segment's last row leaves at once.
__global__ __launch_bounds__(kRowsPerGroup *kWaveLanes) void frames_total_kernel(const RowLaunch R, const float *lat, const float *final_all,
                                                                                   float *frame_total) {
  const int seg = static_cast<int>(blockIdx.y), lane = static_cast<int>(threadIdx.x) % kWaveLanes;
  const int t = static_cast<int>(blockIdx.x) * kRowsPerGroup + static_cast<int>(threadIdx.x) / kWaveLanes;
  const int T = R.T[seg], S = R.S[seg];
  if (t >= T) return;
  const float *row = lat + static_cast<size_t>(R.lat_off[seg]) + static_cast<size_t>(t) * static_cast<size_t>(S);
  const float *final_lp = final_all ? final_all + R.state0[seg] : nullptr;
  const float ninf = float_of(kMinusInf);
  float p[4] = {ninf, ninf, ninf, ninf};
  if (S <= kPartials) {
    // partial i holds state i's term alone: the lane's four final_of values first, once, then the row
    float f[4], x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = lane + k * kWaveLanes < S ? final_of(final_lp, lane + k * kWaveLanes, S) : ninf;
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = lane + k * kWaveLanes < S ? row[lane + k * kWaveLanes] : ninf;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float term = x[k] + f[k];
      if (lane + k * kWaveLanes < S && term == term) p[k] = ladd(p[k], term);
    }
  } else {
    for (int base = 0; base < S; base += kPartials) {
      float x[4], f[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {  // four loads of 64 consecutive floats across the wave, in flight together
        const int j = base + k * kWaveLanes + lane;
        x[k] = j < S ? row[j] : ninf;
        f[k] = j < S ? final_of(final_lp, j, S) : ninf;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float term = x[k] + f[k];
        if (base + k * kWaveLanes + lane < S && term == term) p[k] = ladd(p[k], term);
      }
    }
  }
  p[0] = ladd(p[0], p[2]), p[1] = ladd(p[1], p[3]);  // step 128
  p[0] = ladd(p[0], p[1]);                            // step 64
#pragma unroll
  for (int step = 32; step >= 1; step /= 2) p[0] = ladd(p[0], __shfl_down(p[0], step));  // (lanes below `step` hold the tree's partials)
  if (lane == 0) frame_total[static_cast<size_t>(R.frame_off[seg]) + static_cast<size_t>(t)] = p[0];
}

template <class Kernel>
void launch_wg(Kernel kernel, const Launch &l, const Args &a, hipStream_t s) {
  // 2 x kMaxStates floats: above the 64 KiB a launch gets unasked.  Per device, like every sibling launcher (one mask per
  // kernel instance: the static is this template instance's)
  static std::atomic<unsigned long long> attr_set{0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long dev_bit = 1ull << (dev & 63);
  if (!(attr_set.load(std::memory_order_acquire) & dev_bit)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 2 * kMaxStates);
    attr_set.fetch_or(dev_bit, std::memory_order_release);
  }
  hipLaunchKernelGGL(kernel, dim3(l.n_segs), dim3(kWgThreads), l.lds_bytes, s, l, a);
}

template <int TYPE, bool FREE>
void launch_typed(const Launch &l, const Args &a, hipStream_t s) {
  const dim3 grid(l.n_segs);
  if (l.form == kWorkgroup) {
    launch_wg(frames_wg_kernel<TYPE, FREE>, l, a, s);
    return;
  }
  switch (l.K) {
    case 1: hipLaunchKernelGGL((frames_wave_kernel<1, TYPE, FREE>), grid, dim3(kWaveLanes), l.lds_bytes, s, l, a); break;
    case 2: hipLaunchKernelGGL((frames_wave_kernel<2, TYPE, FREE>), grid, dim3(kWaveLanes), l.lds_bytes, s, l, a); break;
    default: hipLaunchKernelGGL((frames_wave_kernel<4, TYPE, FREE>), grid, dim3(kWaveLanes), l.lds_bytes, s, l, a); break;
  }
}

template <bool FREE>
void launch_free(const Launch &l, const Args &a, int type, hipStream_t s) {
  if (type == kScores) launch_typed<kScores, FREE>(l, a, s);
  else if (type == loglik::kF16) launch_typed<loglik::kF16, FREE>(l, a, s);
  else launch_typed<loglik::kF32, FREE>(l, a, s);
}

}  // namespace

void launch_fb_frames(const fb_frames::Plan &p, const FbFramesArgs &g, hipStream_t s) {
  const Args a{g.d_rows,     g.d_col,      g.d_state_node, g.d_log_prior, g.width,     g.floor,     g.d_arc_ptr,    g.d_arc_src,
               g.d_arc_lp,   g.d_start_lp, g.d_final_lp,   g.d_alpha_in,  g.d_alpha_out, g.d_scratch, g.d_frame_total};
  for (size_t i = 0; i < p.sweep.launches.size(); ++i) {
    const Launch &l = p.sweep.launches[i];
    const RowLaunch &r = p.rows[i];
    g_frames_launches.bump(l.form == kWave ? 0 : 1);
    if (g.free_start) launch_free<true>(l, a, g.type, s);
    else launch_free<false>(l, a, g.type, s);
    g_frames_launches.bump(2);
    const dim3 grid(static_cast<unsigned>((r.max_T + kRowsPerGroup - 1) / kRowsPerGroup), static_cast<unsigned>(r.n_segs));
    hipLaunchKernelGGL(frames_total_kernel, grid, dim3(kRowsPerGroup * kWaveLanes), 0, s, r, g.d_scratch, g.d_final_lp, g.d_frame_total);
  }
}

void fb_frames_launch_counts(unsigned long long out[3]) { g_frames_launches.read(out); }

}  // namespace fdnn
