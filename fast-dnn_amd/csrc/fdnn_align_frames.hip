// fdnn_align_frames.hip -- ALIGNMENT GRAPHS, BEST PATH, FRAME BY FRAME: at every frame of a segment the best path's score, the
// state it ends in and the frame it began at, with a start that may be free and a row carried from one call to the next
// (fdnn_align_frames.hpp: the contract, the plan and the host restatement; the arithmetic is fdnn_align_graph.hpp's relax and
// better_end and align::emission, called from here).
//
//   The caller who follows a live utterance with a keyword graph had one fdnn_calculate_align_graph call per prefix and per
//   candidate start, or the summed frames form, which has no begin frame.
//
// ONE launch per form; no lattice, no back-pointers, no scratch.  A token carries its path's begin frame: b lives beside d as
// two int32 LDS rows, swapped together, and the per-frame selection -- a compare and select, no chain of log-adds -- rides
// inside the sweep, off the step's dependent chain.
//
// frames_wave_kernel<K, TYPE, FREE>: one wave per segment, S <= 64 K <= kWaveStates.  Lane l owns states l, l + 64, .. and keeps
//   their column, prior, start_of and final_of values in registers; the loads of the next 16 / K rows are in flight while the
//   current ones are stepped, their emissions waiting in an LDS ring; the arc offsets, and the arc table where it has at most
//   kArcLdsArcs arcs, are staged in LDS once; no workgroup barrier.  As a lane steps frame u of a group it folds its K states'
//   (d + final, j, b) into one triple for that frame and keeps the group's D triples in registers; after the group's last step
//   the D frames are reduced together over the 64 lanes -- six cross-lane steps, D independent reductions interleaved -- and
//   lane 0 stores the group's frame_best / frame_end / frame_begin.
// frames_wg_kernel<TYPE, FREE>: 256 threads per segment, any S <= align_frames::kMaxStates; one barrier per frame.  A thread
//   folds its states, its wave reduces, and the wave's triple goes to an LDS slot indexed by frame parity; after the NEXT
//   frame's barrier thread 0 folds the four triples of the frame before and stores them; the last frame's after the loop.
// With carry the first rows of d and b are loaded from d_in / begin_in before anything is stored and frame 0 takes the
// ordinary step; d_out / begin_out are stored last, by the segment's own states only: in place is sound, and a second
// launch's segments touch disjoint words.
// Every arc index is bounded by the HOST table's counts (Launch::arc0 / n_arcs), whatever the device copies hold.
//
// No atomics, no inline assembly, no device state that outlives a launch.  Built WITHOUT a flush-to-zero or fast-math flag,
// with -ffp-contract=off and without the packed fp32 forms (csrc/Makefile): the header's sequence is what runs.
#include "fdnn_device.hpp"
#include "fdnn_kernels.hpp"
#include "fdnn_launch.hpp"
#include "fdnn_align_frames.hpp"

namespace fdnn {
namespace {

using namespace align_frames;
using align_graph::frames_in_flight;
using align_graph::kWave;
using align_graph::kWorkgroup;
using align_graph::Launch;

LaunchCounts<2> g_frames_launches;  // wave form, workgroup form

struct Args {
  const float *rows;
  const int32_t *col, *node;  // node: null without a handle
  const float *prior;         // the handle's log priors [width]
  int width;
  float floor;
  const int32_t *ptr, *src;
  const float *lp;
  const float *start_lp, *final_lp;  // null = state 0 / state S - 1
  const float *d_in;                 // [states of the call] or null, with begin_in
  const int32_t *begin_in;
  float *d_out;  // each the same shape, or null
  int32_t *begin_out;
  float *frame_best;
  int32_t *frame_end, *frame_begin;
};

// frame_base of the launch's segments, from the host table: a kernel argument by value beside the Launch
struct Bases {
  int32_t v[kMaxSegs];
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
// column 0 of the row (inside it: ld >= 1) and the value is made a NaN by its bits, as in the siblings
__device__ __forceinline__ float row_value(const float *rows, int t, int ld, int col) {
  const int bad = col >> 31;  // 0 or all ones
  const float v = rows[static_cast<size_t>(t) * static_cast<size_t>(ld) + static_cast<size_t>(col & ~bad)];
  return float_of(bits_of(v) | (static_cast<uint32_t>(bad) & kQuietNaN));
}

// a frame's selection
struct Triple {
  float best;
  int end;
  int32_t bg;
};
__device__ __forceinline__ Triple nothing() { return Triple{float_of(kMinusInf), -1, -1}; }

// N triples over a wave's lanes, the N reductions interleaved: fold is order-free, and the lanes' indices are distinct
template <int N>
__device__ __forceinline__ void wave_select(Triple (&q)[N]) {
#pragma unroll
  for (int m = 1; m < kWaveLanes; m *= 2) {
    Triple o[N];
#pragma unroll
    for (int u = 0; u < N; ++u) o[u] = Triple{__shfl_xor(q[u].best, m), __shfl_xor(q[u].end, m), __shfl_xor(q[u].bg, m)};
#pragma unroll
    for (int u = 0; u < N; ++u) fold(o[u].best, o[u].end, o[u].bg, &q[u].best, &q[u].end, &q[u].bg);
  }
}

__device__ __forceinline__ void store_frame(const Args &a, size_t at, const Triple &q) {
  a.frame_best[at] = float_of(align::total_bits(q.best));
  a.frame_end[at] = q.end;
  a.frame_begin[at] = q.end >= 0 ? q.bg : -1;
}

// The wave form's frames first .. T - 1, stepped from the rows in cur / curb.  Frames go in groups of D = frames_in_flight(K):
// the group's emissions are put into the LDS ring from the values that came in during the group before, the loads of the
// NEXT group are issued, the group's frames are stepped and folded, and the group's D selections are reduced together.
template <int K, int TYPE, bool FREE, bool STAGED>
__device__ __forceinline__ void wave_frames(const Args &a, const float *rows, size_t out, int32_t base, int first, int T, int S, int ld, int lane,
                                            int arc0, const int (&col)[K], const float (&prior)[K], const float (&start)[K], const float (&fin)[K],
                                            float *cur, float *nxt, int32_t *curb, int32_t *nxtb, float *em, const int *abeg, const float *alp,
                                            const uint16_t *asrc, float **last, int32_t **lastb) {
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
    Triple q[D];
#pragma unroll
    for (int u = 0; u < D; ++u) {
      q[u] = nothing();
      if (u0 + u < T) {  // (uniform)
        const int t = u0 + u;
        const float *e = em + u * K * kWaveLanes;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int j = lane + k * kWaveLanes;
          if (j < S) {
            const int a0 = abeg[j], a1 = abeg[j + 1];
            float best = ninf;
            int from = -1;
            for (int i = a0; i < a1; ++i) {
              int src;
              float lp;
              if constexpr (STAGED) {
                src = asrc[i], lp = alp[i];
              } else {
                src = a.src[arc0 + i], lp = a.lp[arc0 + i];
              }
              relax(static_cast<unsigned>(src) < static_cast<unsigned>(S) ? cur[src] : nan, lp, src, &best, &from);
            }
            // (a taken source is inside [0, S): an outside one is a NaN candidate -- the staged kNoSource included)
            int32_t bg;
            after_arcs(from, from >= 0 ? curb[from] : -1, FREE, start[k], frame_no(base, t), &best, &bg);
            const float val = best + e[j];
            nxt[j] = val, nxtb[j] = bg;
            fold(val + fin[k], j, bg, &q[u].best, &q[u].end, &q[u].bg);  // (off the chain: nothing of the next frame reads it)
          }
        }
        wave_sync();
        float *sw = cur;
        cur = nxt, nxt = sw;
        int32_t *swb = curb;
        curb = nxtb, nxtb = swb;
      }
    }
    wave_select<D>(q);
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < D; ++u)
        if (u0 + u < T) store_frame(a, out + static_cast<size_t>(u0 + u), q[u]);
    }
  }
  *last = cur, *lastb = curb;
}

template <int K, int TYPE, bool FREE>
__global__ __launch_bounds__(kWaveLanes) void frames_wave_kernel(const Launch L, const Bases B, const Args a) {
  extern __shared__ uint32_t lds32[];
  const int seg = static_cast<int>(blockIdx.x), lane = static_cast<int>(threadIdx.x);
  const int T = L.T[seg], S = L.S[seg], ld = L.ld[seg], s0 = L.state0[seg], arc0 = L.arc0[seg], n_arcs = L.n_arcs[seg];
  const int32_t base = B.v[seg];
  const float *rows = a.rows + L.row_off[seg];
  const size_t out = static_cast<size_t>(L.path_off[seg]);
  float *cur = reinterpret_cast<float *>(lds32), *nxt = cur + L.d_floats;
  int32_t *curb = reinterpret_cast<int32_t *>(nxt + L.d_floats), *nxtb = curb + L.d_floats;
  float *em = reinterpret_cast<float *>(nxtb + L.d_floats);
  int *abeg = reinterpret_cast<int *>(em + kEmissionRing);
  float *alp = reinterpret_cast<float *>(abeg + L.d_floats + 64);
  uint16_t *asrc = reinterpret_cast<uint16_t *>(alp + L.arc_cap);
  const bool staged = n_arcs <= L.arc_cap;  // (the plan's rule: arc_cap is the largest staged count of the launch, at most kArcLdsArcs)
  const bool carried = a.d_in != nullptr;

  // the arc offsets, local to the segment and inside the host table's count whatever the device copy holds
  for (int j = lane; j <= S; j += kWaveLanes) abeg[j] = clampi(a.ptr[s0 + j] - arc0, 0, n_arcs);
  if (staged)
    for (int i = lane; i < n_arcs; i += kWaveLanes) {
      const int src = a.src[arc0 + i];
      alp[i] = a.lp[arc0 + i];
      asrc[i] = static_cast<unsigned>(src) < static_cast<unsigned>(S) ? static_cast<uint16_t>(src) : align_graph::kNoSource;
    }

  // slot k of a lane is state lane + 64 k (64 K >= the launch's largest graph, so the rows hold every slot); the slots past S
  // have column -1 and hold NaNs nothing reads.  The first rows: the carry, or the start row, which is frame 0's
  int col[K];
  float prior[K], start[K], fin[K];
  Triple q0[1] = {nothing()};
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int j = lane + k * kWaveLanes;
    const State st = load_state<TYPE>(a, s0 + j, j < S, ld);
    col[k] = st.col, prior[k] = st.prior;
    start[k] = j < S ? start_of(a.start_lp ? a.start_lp + s0 : nullptr, j) : float_of(kMinusInf);
    fin[k] = j < S ? final_of(a.final_lp ? a.final_lp + s0 : nullptr, j, S) : float_of(kMinusInf);
    if (carried) {
      cur[j] = j < S ? a.d_in[s0 + j] : float_of(kQuietNaN);
      curb[j] = j < S ? a.begin_in[s0 + j] : -1;
    } else {
      const float val = start[k] + align::emission(row_value(rows, 0, ld, col[k]), prior[k], a.floor, TYPE);
      const int32_t bg = start_begin(start[k], base);
      cur[j] = val, curb[j] = bg;
      if (j < S) fold(val + fin[k], j, bg, &q0[0].best, &q0[0].end, &q0[0].bg);
    }
  }
  if (!carried) {
    wave_select<1>(q0);
    if (lane == 0) store_frame(a, out, q0[0]);
  }
  wave_sync();
  float *last = cur;
  int32_t *lastb = curb;
  const int first = carried ? 0 : 1;
  if (staged)
    wave_frames<K, TYPE, FREE, true>(a, rows, out, base, first, T, S, ld, lane, arc0, col, prior, start, fin, cur, nxt, curb, nxtb, em, abeg, alp, asrc,
                                     &last, &lastb);
  else
    wave_frames<K, TYPE, FREE, false>(a, rows, out, base, first, T, S, ld, lane, arc0, col, prior, start, fin, cur, nxt, curb, nxtb, em, abeg, alp, asrc,
                                      &last, &lastb);
  if (a.d_out)
    for (int j = lane; j < S; j += kWaveLanes) a.d_out[s0 + j] = last[j];
  if (a.begin_out)
    for (int j = lane; j < S; j += kWaveLanes) a.begin_out[s0 + j] = lastb[j];
}

template <int TYPE, bool FREE>
__global__ __launch_bounds__(kWgThreads) void frames_wg_kernel(const Launch L, const Bases B, const Args a) {
  extern __shared__ uint32_t lds32[];
  constexpr int kWaves = kWgThreads / kWaveLanes;
  const int seg = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x);
  const int T = L.T[seg], S = L.S[seg], ld = L.ld[seg], s0 = L.state0[seg], arc0 = L.arc0[seg], n_arcs = L.n_arcs[seg];
  const int32_t base = B.v[seg];
  const float *rows = a.rows + L.row_off[seg];
  const size_t out = static_cast<size_t>(L.path_off[seg]);
  float *cur = reinterpret_cast<float *>(lds32), *nxt = cur + L.d_floats;
  int32_t *curb = reinterpret_cast<int32_t *>(nxt + L.d_floats), *nxtb = curb + L.d_floats;
  uint32_t *slot = reinterpret_cast<uint32_t *>(nxtb + L.d_floats);  // [parity][wave][3]
  const float ninf = float_of(kMinusInf), nan = float_of(kQuietNaN);
  const float *start_lp = a.start_lp ? a.start_lp + s0 : nullptr, *final_lp = a.final_lp ? a.final_lp + s0 : nullptr;
  const bool carried = a.d_in != nullptr;

  // the four waves' triples of frame t, by one thread, after the barrier behind frame t
  auto finish_frame = [&](int t) {
    const uint32_t *w = slot + (t & 1) * 3 * kWaves;
    Triple q = nothing();
    for (int i = 0; i < kWaves; ++i) fold(float_of(w[3 * i]), static_cast<int>(w[3 * i + 1]), static_cast<int32_t>(w[3 * i + 2]), &q.best, &q.end, &q.bg);
    store_frame(a, out + static_cast<size_t>(t), q);
  };

  if (carried) {
    for (int j = tid; j < S; j += kWgThreads) cur[j] = a.d_in[s0 + j], curb[j] = a.begin_in[s0 + j];
    __syncthreads();
  }
  for (int t = 0; t < T; ++t) {
    if (tid == 0 && t > 0) finish_frame(t - 1);
    Triple q[1] = {nothing()};
    for (int j = tid; j < S; j += kWgThreads) {
      const State st = load_state<TYPE>(a, s0 + j, true, ld);
      const float v = st.col >= 0 ? rows[static_cast<size_t>(t) * static_cast<size_t>(ld) + static_cast<size_t>(st.col)] : nan;
      const float e = align::emission(v, st.prior, a.floor, TYPE);  // (does not depend on d)
      const float start = start_of(start_lp, j);
      float best;
      int32_t bg;
      if (t == 0 && !carried) {
        best = start, bg = start_begin(start, base);
      } else {
        const int a0 = clampi(a.ptr[s0 + j] - arc0, 0, n_arcs), a1 = clampi(a.ptr[s0 + j + 1] - arc0, a0, n_arcs);
        best = ninf;
        int from = -1;
        for (int i = a0; i < a1; ++i) {
          const int src = a.src[arc0 + i];
          relax(static_cast<unsigned>(src) < static_cast<unsigned>(S) ? cur[src] : nan, a.lp[arc0 + i], src, &best, &from);
        }
        after_arcs(from, from >= 0 ? curb[from] : -1, FREE, start, frame_no(base, t), &best, &bg);
      }
      const float val = best + e;
      nxt[j] = val, nxtb[j] = bg;
      fold(val + final_of(final_lp, j, S), j, bg, &q[0].best, &q[0].end, &q[0].bg);
    }
    wave_select<1>(q);
    if ((tid & (kWaveLanes - 1)) == 0) {
      uint32_t *w = slot + (t & 1) * 3 * kWaves + 3 * (tid / kWaveLanes);
      w[0] = bits_of(q[0].best), w[1] = static_cast<uint32_t>(q[0].end), w[2] = static_cast<uint32_t>(q[0].bg);
    }
    __syncthreads();
    float *sw = cur;
    cur = nxt, nxt = sw;
    int32_t *swb = curb;
    curb = nxtb, nxtb = swb;
  }
  if (tid == 0) finish_frame(T - 1);
  if (a.d_out)
    for (int j = tid; j < S; j += kWgThreads) a.d_out[s0 + j] = cur[j];
  if (a.begin_out)
    for (int j = tid; j < S; j += kWgThreads) a.begin_out[s0 + j] = curb[j];
}

// 4 x kMaxStates words: above the 64 KiB a launch gets unasked.  Per device and PER KERNEL INSTANCE: the six instances share one
// function type, so the instance is a template parameter of its own and the static mask is that instance's alone
template <int TYPE, bool FREE>
void launch_wg(const Launch &l, const Bases &b, const Args &a, hipStream_t s) {
  static std::atomic<unsigned long long> attr_set{0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long dev_bit = 1ull << (dev & 63);
  if (!(attr_set.load(std::memory_order_acquire) & dev_bit)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(frames_wg_kernel<TYPE, FREE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              4 * wg_lds_words(kMaxStates));
    attr_set.fetch_or(dev_bit, std::memory_order_release);
  }
  hipLaunchKernelGGL((frames_wg_kernel<TYPE, FREE>), dim3(l.n_segs), dim3(kWgThreads), l.lds_bytes, s, l, b, a);
}

template <int TYPE, bool FREE>
void launch_typed(const Launch &l, const Bases &b, const Args &a, hipStream_t s) {
  const dim3 grid(l.n_segs);
  if (l.form == kWorkgroup) {
    launch_wg<TYPE, FREE>(l, b, a, s);
    return;
  }
  switch (l.K) {
    case 1: hipLaunchKernelGGL((frames_wave_kernel<1, TYPE, FREE>), grid, dim3(kWaveLanes), l.lds_bytes, s, l, b, a); break;
    case 2: hipLaunchKernelGGL((frames_wave_kernel<2, TYPE, FREE>), grid, dim3(kWaveLanes), l.lds_bytes, s, l, b, a); break;
    default: hipLaunchKernelGGL((frames_wave_kernel<4, TYPE, FREE>), grid, dim3(kWaveLanes), l.lds_bytes, s, l, b, a); break;
  }
}

template <bool FREE>
void launch_free(const Launch &l, const Bases &b, const Args &a, int type, hipStream_t s) {
  if (type == kScores) launch_typed<kScores, FREE>(l, b, a, s);
  else if (type == loglik::kF16) launch_typed<loglik::kF16, FREE>(l, b, a, s);
  else launch_typed<loglik::kF32, FREE>(l, b, a, s);
}

}  // namespace

void launch_align_frames(const align_graph::Plan &p, const AlignFramesArgs &g, hipStream_t s) {
  const Args a{g.d_rows,     g.d_col,      g.d_state_node, g.d_log_prior, g.width,   g.floor,       g.d_arc_ptr,    g.d_arc_src,  g.d_arc_lp,     g.d_start_lp,
               g.d_final_lp, g.d_d_in,     g.d_begin_in,   g.d_d_out,     g.d_begin_out, g.d_frame_best, g.d_frame_end, g.d_frame_begin};
  for (const Launch &l : p.launches) {
    Bases b{};
    for (int i = 0; i < l.n_segs; ++i) b.v[i] = g.frame_base ? g.frame_base[l.total_off[i]] : 0;
    g_frames_launches.bump(l.form == kWave ? 0 : 1);
    if (g.free_start) launch_free<true>(l, b, a, g.type, s);
    else launch_free<false>(l, b, a, g.type, s);
  }
}

void align_frames_launch_counts(unsigned long long out[2]) { g_frames_launches.read(out); }

}  // namespace fdnn
