// fdnn_align_graph.hip -- ALIGNMENT GRAPHS: the best path over any arc set of a segment's states, and its score
// (fdnn_align_graph.hpp: the candidate step, the final selection, the plan, the host restatement -- the arithmetic is the
// headers', called from here; the emission is the sibling's, align::emission).
//
//   The caller of LazyOutputActivations (dnn.cc:355-392) whose transcript is no strict chain -- optional silence,
//   pronunciation variants, a keyword against a filler -- had the sibling's forced silences or the host's Viterbi.
//
// The row loop is sequential in t.  A source is any state, so the chain form's register / DPP hand-off does not carry over:
// d lives as two rows in LDS in both forms, and what a frame's chain holds is one LDS read, one addition, one compare and
// select per arc, one addition and one LDS write per state.
//
// graph_wave_kernel<K, TYPE>: one wave per segment, S <= 64 K <= kWaveStates.  Lane l owns states l, l + 64, .. (slot k = state
// l + 64 k): their column and prior live in registers.  Emissions do not depend on d: the loads of the next 16 / K rows are
// issued, and the emissions of the current ones are scored into an LDS ring, before the steps that consume them, so no frame
// waits for the L2 (the workgroup form pays one L2 round trip a frame).  The arc offsets [S + 1], and the arc table (score 4
// bytes, source 2) where the segment has at most kArcLdsArcs arcs, are staged in LDS once; a larger table is read from the L2
// every frame.  No workgroup barrier: the wave's own LDS accesses are served in order, so between the frames there is a
// wave-scope fence for the compiler and nothing for the hardware to wait on.
// graph_wg_kernel<TYPE>: 256 threads per segment, any S <= kMaxStates; thread i owns states i, i + 256, ..; one barrier per
// frame; column, node, prior, arc offsets and arcs are read again every frame (the L2 serves them), as the sibling's
// workgroup form does.
// Back-pointers: the source state per (frame, state) in 16 bits, in LDS where the segment's fit (kBpLdsWords), else in the
// call's scratch (written through to the L2, read back after a fence).  The back-trace is one dependent read per frame by
// one lane.
// Every arc index is bounded by the HOST table's counts (Launch::arc0 / n_arcs), whatever the device copy of arc_ptr holds.
//
// No atomics, no inline assembly, no device state that outlives a launch.  Built WITHOUT a flush-to-zero or fast-math flag
// and with -ffp-contract=off (csrc/Makefile): the header's sequence is what runs.
#include "fdnn_device.hpp"
#include "fdnn_kernels.hpp"
#include "fdnn_launch.hpp"
#include "fdnn_align_graph.hpp"

namespace fdnn {
namespace {

using namespace align_graph;

LaunchCounts<2> g_graph_launches;  // wave form, workgroup form
std::atomic<int> g_graph_mode{0};  // fdnn_debug_set_align_graph_kernel

struct Args {
  const float *rows;
  const int32_t *col, *node;  // node: null without a handle
  const float *prior;         // the handle's log priors [width]
  int width;
  float floor;
  const int32_t *arc_ptr, *arc_src;
  const float *arc_lp, *start_lp, *final_lp;  // start_lp, final_lp: null = state 0 / state S - 1
  uint32_t *scratch;
  int32_t *path;
  float *total;
};

// what a thread keeps of one state: the column (-1 unless the state exists and its column and node are in range) and the prior
struct State {
  int col;
  float prior;
  __device__ bool valid() const { return col >= 0; }
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

// (best, end) over a wave's lanes: better_end is the maximum under > and the lowest index among its equals, in any order
__device__ inline void wave_best(float *best, int *end) {
#pragma unroll
  for (int m = 1; m < kWaveLanes; m *= 2) {
    const float ob = __shfl_xor(*best, m);
    const int oe = __shfl_xor(*end, m);
    better_end(ob, oe, best, end);
  }
}

// (the callers have made the back-pointers visible: a fence and a barrier)
__device__ inline void finish(const Launch &L, int seg, const Args &a, float tot, int end, const uint16_t *bp, bool first_thread) {
  const int T = L.T[seg], S = L.S[seg];
  int32_t *path = a.path + L.path_off[seg];
  const uint32_t tb = align::total_bits(tot);
  if (!finite_bits(tb)) {
    for (int t = static_cast<int>(threadIdx.x); t < T; t += static_cast<int>(blockDim.x)) path[t] = -1;
  } else if (first_thread) {
    int j = end;
    for (int t = T - 1; t >= 1; --t) {
      path[t] = j;
      j = min(static_cast<int>(bp[static_cast<size_t>(t) * static_cast<size_t>(S) + static_cast<size_t>(j)]), S - 1);
    }
    path[0] = j;
  }
  if (first_thread) a.total[L.total_off[seg]] = float_of(tb);
}

// A slot's value of row t.  col is -1 where the slot has no state or the state's column or node is out of range: the load
// then goes to column 0 of the row (inside it: ld >= 1) and the value is made a NaN by its bits -- a compare per slot would
// be a lane mask per slot, held in scalar registers across the row loop.  (The payload of that NaN is never seen: a NaN is
// never taken, so it reaches neither a path nor a total.)
__device__ __forceinline__ float row_value(const float *rows, int t, int ld, int col) {
  const int bad = col >> 31;  // 0 or all ones
  const float v = rows[static_cast<size_t>(t) * static_cast<size_t>(ld) + static_cast<size_t>(col & ~bad)];
  return float_of(bits_of(v) | (static_cast<uint32_t>(bad) & kQuietNaN));
}

// the wave form's frames; K: states per lane; STAGED: the arc table is in LDS (sources in 16 bits, kNoSource where outside [0, S)).
// Frames go in groups of D = frames_in_flight(K): the group's emissions are scored into the LDS ring from the values that
// came in during the group before, the loads of the NEXT group are issued, and then the group's frames are stepped -- so
// no step waits for the L2.
template <int K, int TYPE, bool STAGED>
__device__ __forceinline__ void wave_frames(const Args &a, const float *rows, int T, int S, int ld, int lane, int arc0, const int (&col)[K],
                                            const float (&prior)[K], float *cur, float *nxt, float *em, const int *abeg, const float *alp,
                                            const uint16_t *asrc, uint16_t *bp, float **last) {
  constexpr int D = frames_in_flight(K);
  const float ninf = float_of(kMinusInf), nan = float_of(kQuietNaN);
  float v[D][K];
#pragma unroll
  for (int u = 0; u < D; ++u)
#pragma unroll
    for (int k = 0; k < K; ++k) v[u][k] = 1 + u < T ? row_value(rows, 1 + u, ld, col[k]) : nan;  // (uniform)
  for (int t0 = 1; t0 < T; t0 += D) {
#pragma unroll
    for (int u = 0; u < D; ++u)
#pragma unroll
      for (int k = 0; k < K; ++k) em[(u * K + k) * kWaveLanes + lane] = align::emission(v[u][k], prior[k], a.floor, TYPE);  // (a lane's own states)
#pragma unroll
    for (int u = 0; u < D; ++u)
      if (t0 + D + u < T) {  // (uniform) in flight during the steps below
#pragma unroll
        for (int k = 0; k < K; ++k) v[u][k] = row_value(rows, t0 + D + u, ld, col[k]);
      }
#pragma unroll
    for (int u = 0; u < D; ++u) {
      const int t = t0 + u;
      if (t < T) {  // (uniform)
        const float *e = em + u * K * kWaveLanes;
        for (int j = lane; j < S; j += kWaveLanes) {
          const int a0 = abeg[j], a1 = abeg[j + 1];
          float best = ninf;
          int from = -1;
          for (int i = a0; i < a1; ++i) {
            int src;
            float lp;
            if constexpr (STAGED) {
              src = asrc[i], lp = alp[i];
            } else {
              src = a.arc_src[arc0 + i], lp = a.arc_lp[arc0 + i];
            }
            relax(static_cast<unsigned>(src) < static_cast<unsigned>(S) ? cur[src] : nan, lp, src, &best, &from);
          }
          nxt[j] = best + e[j];
          bp[static_cast<size_t>(t) * static_cast<size_t>(S) + static_cast<size_t>(j)] = static_cast<uint16_t>(from);
        }
        wave_sync();
        float *sw = cur;
        cur = nxt, nxt = sw;
      }
    }
  }
  *last = cur;
}

template <int K, int TYPE>
__global__ __launch_bounds__(kWaveLanes) void graph_wave_kernel(const Launch L, const Args a) {
  extern __shared__ uint32_t lds32[];
  const int seg = static_cast<int>(blockIdx.x), lane = static_cast<int>(threadIdx.x);
  const int T = L.T[seg], S = L.S[seg], ld = L.ld[seg], s0 = L.state0[seg], arc0 = L.arc0[seg], n_arcs = L.n_arcs[seg];
  const float *rows = a.rows + L.row_off[seg];
  float *cur = reinterpret_cast<float *>(lds32), *nxt = cur + L.d_floats, *em = nxt + L.d_floats;
  int *abeg = reinterpret_cast<int *>(em + kEmissionRing);
  float *alp = reinterpret_cast<float *>(abeg + L.d_floats + 64);
  uint16_t *asrc = reinterpret_cast<uint16_t *>(alp + L.arc_cap);
  uint32_t *bp_lds = reinterpret_cast<uint32_t *>(alp + L.arc_cap) + L.arc_cap / 2;
  uint16_t *bp = L.bp_off[seg] < 0 ? reinterpret_cast<uint16_t *>(bp_lds) : reinterpret_cast<uint16_t *>(a.scratch + L.bp_off[seg]);
  const bool staged = n_arcs <= L.arc_cap;  // (the plan's rule: arc_cap is the largest staged count of the launch, at most kArcLdsArcs)

  // the arc offsets, local to the segment and inside the host table's count whatever the device copy holds
  for (int j = lane; j <= S; j += kWaveLanes) abeg[j] = clampi(a.arc_ptr[s0 + j] - arc0, 0, n_arcs);
  if (staged)
    for (int i = lane; i < n_arcs; i += kWaveLanes) {
      const int src = a.arc_src[arc0 + i];
      alp[i] = a.arc_lp[arc0 + i];
      asrc[i] = static_cast<unsigned>(src) < static_cast<unsigned>(S) ? static_cast<uint16_t>(src) : kNoSource;
    }

  // slot k of a lane is state lane + 64 k (64 K >= the launch's largest graph, so d's rows hold every slot); the slots past S
  // have column -1: NaNs nothing reads
  int col[K];
  float prior[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int j = lane + k * kWaveLanes;
    const State st = load_state<TYPE>(a, s0 + j, j < S, ld);
    col[k] = st.col, prior[k] = st.prior;
    const float start = j < S ? start_of(a.start_lp ? a.start_lp + s0 : nullptr, j) : 0.0f;
    cur[j] = start + align::emission(row_value(rows, 0, ld, col[k]), prior[k], a.floor, TYPE);
  }
  wave_sync();
  float *last = cur;
  if (staged) wave_frames<K, TYPE, true>(a, rows, T, S, ld, lane, arc0, col, prior, cur, nxt, em, abeg, alp, asrc, bp, &last);
  else wave_frames<K, TYPE, false>(a, rows, T, S, ld, lane, arc0, col, prior, cur, nxt, em, abeg, alp, asrc, bp, &last);

  // the total: each lane over its states in ascending order, then over the lanes
  float best = float_of(kMinusInf);
  int end = -1;
  for (int j = lane; j < S; j += kWaveLanes) better_end(last[j] + final_of(a.final_lp ? a.final_lp + s0 : nullptr, j, S), j, &best, &end);
  wave_best(&best, &end);
  __threadfence();
  __syncthreads();
  finish(L, seg, a, best, end, bp, lane == 0);
}

template <int TYPE>
__global__ __launch_bounds__(kWgThreads) void graph_wg_kernel(const Launch L, const Args a) {
  extern __shared__ uint32_t lds32[];
  const int seg = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x);
  const int T = L.T[seg], S = L.S[seg], ld = L.ld[seg], s0 = L.state0[seg], arc0 = L.arc0[seg], n_arcs = L.n_arcs[seg];
  const float *rows = a.rows + L.row_off[seg];
  float *cur = reinterpret_cast<float *>(lds32), *nxt = cur + L.d_floats;
  uint32_t *red = reinterpret_cast<uint32_t *>(nxt + L.d_floats);
  uint16_t *bp = L.bp_off[seg] < 0 ? reinterpret_cast<uint16_t *>(red + kWgReduceWords) : reinterpret_cast<uint16_t *>(a.scratch + L.bp_off[seg]);
  const float ninf = float_of(kMinusInf), nan = float_of(kQuietNaN);

  auto emit = [&](int t, int j) {
    const State st = load_state<TYPE>(a, s0 + j, true, ld);
    const float v = st.valid() ? rows[static_cast<size_t>(t) * static_cast<size_t>(ld) + static_cast<size_t>(st.col)] : nan;
    return align::emission(v, st.prior, a.floor, TYPE);
  };
  for (int j = tid; j < S; j += kWgThreads) cur[j] = start_of(a.start_lp ? a.start_lp + s0 : nullptr, j) + emit(0, j);
  __syncthreads();
  for (int t = 1; t < T; ++t) {
    for (int j = tid; j < S; j += kWgThreads) {
      const float e = emit(t, j);  // (does not depend on d)
      const int a0 = clampi(a.arc_ptr[s0 + j] - arc0, 0, n_arcs), a1 = clampi(a.arc_ptr[s0 + j + 1] - arc0, a0, n_arcs);
      float best = ninf;
      int from = -1;
      for (int i = a0; i < a1; ++i) {
        const int src = a.arc_src[arc0 + i];
        relax(static_cast<unsigned>(src) < static_cast<unsigned>(S) ? cur[src] : nan, a.arc_lp[arc0 + i], src, &best, &from);
      }
      nxt[j] = best + e;
      bp[static_cast<size_t>(t) * static_cast<size_t>(S) + static_cast<size_t>(j)] = static_cast<uint16_t>(from);
    }
    __syncthreads();
    float *sw = cur;
    cur = nxt, nxt = sw;
  }
  // the total: each thread over its states in ascending order, each wave over its lanes, thread 0 over the four waves
  float best = ninf;
  int end = -1;
  for (int j = tid; j < S; j += kWgThreads) better_end(cur[j] + final_of(a.final_lp ? a.final_lp + s0 : nullptr, j, S), j, &best, &end);
  wave_best(&best, &end);
  if ((tid & (kWaveLanes - 1)) == 0) red[2 * (tid / kWaveLanes)] = bits_of(best), red[2 * (tid / kWaveLanes) + 1] = static_cast<uint32_t>(end);
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kWgThreads / kWaveLanes; ++w) better_end(float_of(red[2 * w]), static_cast<int>(red[2 * w + 1]), &best, &end);
    red[8] = bits_of(best), red[9] = static_cast<uint32_t>(end);
  }
  __threadfence();
  __syncthreads();
  finish(L, seg, a, float_of(red[8]), static_cast<int>(red[9]), bp, tid == 0);
}

template <class Kernel>
void launch_wg(Kernel kernel, const Launch &l, const Args &a, hipStream_t s) {
  // 2 x kMaxStates floats and the back-pointers: above the 64 KiB a launch gets unasked.  Per device, like every sibling
  // launcher (one mask per kernel instance: the static is this template instance's)
  static std::atomic<unsigned long long> attr_set{0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long dev_bit = 1ull << (dev & 63);
  if (!(attr_set.load(std::memory_order_acquire) & dev_bit)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * wg_lds_words(kMaxStates, kBpLdsWords));
    attr_set.fetch_or(dev_bit, std::memory_order_release);
  }
  hipLaunchKernelGGL(kernel, dim3(l.n_segs), dim3(kWgThreads), l.lds_bytes, s, l, a);
}

template <int TYPE>
void launch_typed(const Launch &l, const Args &a, hipStream_t s) {
  const dim3 grid(l.n_segs);
  if (l.form == kWorkgroup) {
    launch_wg(graph_wg_kernel<TYPE>, l, a, s);
    return;
  }
  switch (l.K) {
    case 1: hipLaunchKernelGGL((graph_wave_kernel<1, TYPE>), grid, dim3(kWaveLanes), l.lds_bytes, s, l, a); break;
    case 2: hipLaunchKernelGGL((graph_wave_kernel<2, TYPE>), grid, dim3(kWaveLanes), l.lds_bytes, s, l, a); break;
    default: hipLaunchKernelGGL((graph_wave_kernel<4, TYPE>), grid, dim3(kWaveLanes), l.lds_bytes, s, l, a); break;
  }
}

}  // namespace

void launch_align_graph(const align_graph::Plan &p, const AlignGraphArgs &g, hipStream_t s) {
  const Args a{g.d_rows, g.d_col, g.d_state_node, g.d_log_prior, g.width, g.floor, g.d_arc_ptr, g.d_arc_src, g.d_arc_lp, g.d_start_lp, g.d_final_lp,
               g.d_scratch, g.d_path, g.d_total};
  for (const Launch &l : p.launches) {
    g_graph_launches.bump(l.form == kWave ? 0 : 1);
    if (g.type == kScores) launch_typed<kScores>(l, a, s);
    else if (g.type == loglik::kF16) launch_typed<loglik::kF16>(l, a, s);
    else launch_typed<loglik::kF32>(l, a, s);
  }
}

void align_graph_launch_counts(unsigned long long out[2]) { g_graph_launches.read(out); }
int align_graph_kernel_mode() { return g_graph_mode.load(std::memory_order_relaxed); }
void align_graph_kernel_mode(int mode) { g_graph_mode.store(mode, std::memory_order_relaxed); }

}  // namespace fdnn
