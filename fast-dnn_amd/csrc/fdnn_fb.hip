// fdnn_fb.hip -- ALIGNMENT GRAPHS, SUMMED: the likelihood of a segment's whole graph, ln of the sum over its paths, and the
// state occupancies gamma[t][j] (fdnn_fb.hpp: exp_neg, ladd, the candidate step, the occupancy, the total's order, the plan,
// the host restatement -- the arithmetic is the headers', called from here; the emission is align::emission, the logarithm
// loglik::ln).
//
//   The caller of LazyOutputActivations (dnn.cc:355-392) who needs a keyword's likelihood against a filler's, an
//   utterance's confidence or soft alignments had the lazy sets over PCIe and the host's forward-backward.
//
// ONE kernel body per form with a direction.  Forward: the sibling's row loop (fdnn_align_graph.hip) with the compare and
// select replaced by a log-add, which makes the chain per arc about forty dependent VALU operations; where gamma is wanted
// every alpha[t][.] also goes to the call's scratch, coalesced, and nothing waits for those stores.  Backward: the same loop
// over the transposed tables from the last frame to the first, started from final_lp; it reads alpha[t][.] and the total
// the forward launch left and writes gamma[t][.] as it goes -- ONE lattice and no third kernel.
//
// fb_wave_kernel<K, TYPE, BWD>: one wave per segment, S <= 64 K <= kWaveStates.  Lane l owns states l, l + 64, ..; d as two
// LDS rows; the loads of the next 16 / K rows (backward: 8 / K rows and their alphas) are in flight while the current ones are
// stepped, their emissions and alphas waiting in LDS rings; the arc offsets, and the arc table where it has at most
// kArcLdsArcs arcs, staged in LDS once; no workgroup barrier.  The total: a lane's slots are partials l, l + 64, l + 128,
// l + 192, so the tree's first two steps stay inside the lane and the rest go over the lanes.
// fb_wg_kernel<TYPE, BWD>: 256 threads per segment, any S <= kMaxStates; thread i owns states i, i + 256, .. and partial i;
// one barrier per frame.
// Every arc index is bounded by the HOST table's counts (Launch::arc0 / n_arcs), whatever the device copies hold.
//
// No atomics, no inline assembly, no device state that outlives a launch.  Built WITHOUT a flush-to-zero or fast-math flag
// and with -ffp-contract=off (csrc/Makefile): the header's sequence is what runs.
#include "fdnn_device.hpp"
#include "fdnn_kernels.hpp"
#include "fdnn_launch.hpp"
#include "fdnn_fb.hpp"

namespace fdnn {
namespace {

using namespace fb;

LaunchCounts<4> g_fb_launches;  // forward wave, forward workgroup, backward wave, backward workgroup
std::atomic<int> g_fb_mode{0};  // fdnn_debug_set_fb_kernel

struct Args {
  const float *rows;
  const int32_t *col, *node;  // node: null without a handle
  const float *prior;         // the handle's log priors [width]
  int width;
  float floor;
  const int32_t *ptr, *src;   // this direction's table: arc_ptr / arc_src forward, t_ptr / t_src backward
  const float *lp;
  const float *init_lp;       // where the sweep starts: start_lp forward, final_lp backward (null = state 0 / state S - 1)
  const float *final_lp;      // forward: the total's terms
  float *lat;                 // forward: where alpha goes (null: not wanted); backward: where it is read
  float *gamma;               // backward
  float *total;               // forward: written; backward: read
};

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

// A slot's value of row t; col is -1 where the slot has no state or its column or node is out of range: the load goes to
// column 0 of the row (inside it: ld >= 1) and the value is made a NaN by its bits, as in the sibling
__device__ __forceinline__ float row_value(const float *rows, int t, int ld, int col) {
  const int bad = col >> 31;  // 0 or all ones
  const float v = rows[static_cast<size_t>(t) * static_cast<size_t>(ld) + static_cast<size_t>(col & ~bad)];
  return float_of(bits_of(v) | (static_cast<uint32_t>(bad) & kQuietNaN));
}

template <bool BWD>
__device__ __forceinline__ float init_of(const float *init_lp, int j, int S) {
  return BWD ? final_of(init_lp, j, S) : start_of(init_lp, j);
}

// what a finished state of frame t leaves outside LDS: forward its alpha in the lattice, backward its occupancy
template <bool BWD>
__device__ __forceinline__ void emit_out(const Args &a, size_t at, float val, float e, float alpha, float total) {
  if constexpr (BWD) a.gamma[at] = gamma_of(alpha, val, e, total);
  else if (a.lat) a.lat[at] = val;  // (uniform)
}

// the wave form's frames after the first; u counts steps, the frame is u forward and T - 1 - u backward.  Steps go in groups
// of D = frames_in_flight(K), backward half as many: the group's emissions (and alphas) are put into the LDS rings from the values that came in
// during the group before, the loads of the NEXT group are issued, and then the group's frames are stepped.
template <int K, int TYPE, bool BWD, bool STAGED>
__device__ __forceinline__ void wave_frames(const Args &a, const float *rows, const float *lat, size_t out, float total, int T, int S, int ld, int lane,
                                            int arc0, const int (&col)[K], const float (&prior)[K], float *cur, float *nxt, float *em, float *ax,
                                            const int *abeg, const float *alp, const uint16_t *asrc, float **last) {
  constexpr int D = BWD ? frames_in_flight(K) / 2 : frames_in_flight(K);  // 16 values a lane in flight either way: backward, half are alphas
  const float ninf = float_of(kMinusInf), nan = float_of(kQuietNaN);
  auto frame = [&](int u) { return BWD ? T - 1 - u : u; };
  float v[D][K], al[D][K];
#pragma unroll
  for (int u = 0; u < D; ++u)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = lane + k * kWaveLanes;
      v[u][k] = 1 + u < T ? row_value(rows, frame(1 + u), ld, col[k]) : nan;  // (uniform)
      if constexpr (BWD) al[u][k] = (1 + u < T && j < S) ? lat[out + static_cast<size_t>(frame(1 + u)) * static_cast<size_t>(S) + static_cast<size_t>(j)] : nan;
      else al[u][k] = 0.0f;
    }
  for (int u0 = 1; u0 < T; u0 += D) {
#pragma unroll
    for (int u = 0; u < D; ++u)
#pragma unroll
      for (int k = 0; k < K; ++k) {
        em[(u * K + k) * kWaveLanes + lane] = align::emission(v[u][k], prior[k], a.floor, TYPE);  // (a lane's own states)
        if constexpr (BWD) ax[(u * K + k) * kWaveLanes + lane] = al[u][k];
      }
#pragma unroll
    for (int u = 0; u < D; ++u)
      if (u0 + D + u < T) {  // (uniform) in flight during the steps below
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int j = lane + k * kWaveLanes;
          v[u][k] = row_value(rows, frame(u0 + D + u), ld, col[k]);
          if constexpr (BWD)
            if (j < S) al[u][k] = lat[out + static_cast<size_t>(frame(u0 + D + u)) * static_cast<size_t>(S) + static_cast<size_t>(j)];
        }
      }
#pragma unroll
    for (int u = 0; u < D; ++u) {
      if (u0 + u < T) {  // (uniform)
        const int t = frame(u0 + u);
        const float *e = em + u * K * kWaveLanes, *x = ax + u * K * kWaveLanes;
        for (int j = lane; j < S; j += kWaveLanes) {
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
          const float val = acc + e[j];
          nxt[j] = val;
          emit_out<BWD>(a, out + static_cast<size_t>(t) * static_cast<size_t>(S) + static_cast<size_t>(j), val, e[j], BWD ? x[j] : 0.0f, total);
        }
        wave_sync();
        float *sw = cur;
        cur = nxt, nxt = sw;
      }
    }
  }
  *last = cur;
}

template <int K, int TYPE, bool BWD>
__global__ __launch_bounds__(kWaveLanes) void fb_wave_kernel(const Launch L, const Args a) {
  extern __shared__ uint32_t lds32[];
  const int seg = static_cast<int>(blockIdx.x), lane = static_cast<int>(threadIdx.x);
  const int T = L.T[seg], S = L.S[seg], ld = L.ld[seg], s0 = L.state0[seg], arc0 = L.arc0[seg], n_arcs = L.n_arcs[seg];
  const float *rows = a.rows + L.row_off[seg];
  const size_t out = static_cast<size_t>(L.out_off[seg]);
  float *cur = reinterpret_cast<float *>(lds32), *nxt = cur + L.d_floats, *em = nxt + L.d_floats, *ax = em + kEmissionRing;
  int *abeg = reinterpret_cast<int *>(ax + kEmissionRing);
  float *alp = reinterpret_cast<float *>(abeg + L.d_floats + 64);
  uint16_t *asrc = reinterpret_cast<uint16_t *>(alp + L.arc_cap);
  const bool staged = n_arcs <= L.arc_cap;  // (the plan's rule: arc_cap is the largest staged count of the launch, at most kArcLdsArcs)
  const float total = BWD ? a.total[L.total_off[seg]] : 0.0f;

  // the arc offsets, local to the segment and inside the host table's count whatever the device copy holds
  for (int j = lane; j <= S; j += kWaveLanes) abeg[j] = clampi(a.ptr[s0 + j] - arc0, 0, n_arcs);
  if (staged)
    for (int i = lane; i < n_arcs; i += kWaveLanes) {
      const int src = a.src[arc0 + i];
      alp[i] = a.lp[arc0 + i];
      asrc[i] = static_cast<unsigned>(src) < static_cast<unsigned>(S) ? static_cast<uint16_t>(src) : align_graph::kNoSource;
    }

  // slot k of a lane is state lane + 64 k (64 K >= the launch's largest graph, so d's rows hold every slot); the slots past S
  // have column -1: NaNs nothing reads
  const int t0 = BWD ? T - 1 : 0;
  int col[K];
  float prior[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int j = lane + k * kWaveLanes;
    const State st = load_state<TYPE>(a, s0 + j, j < S, ld);
    col[k] = st.col, prior[k] = st.prior;
    const float init = j < S ? init_of<BWD>(a.init_lp ? a.init_lp + s0 : nullptr, j, S) : 0.0f;
    const float e = align::emission(row_value(rows, t0, ld, col[k]), prior[k], a.floor, TYPE);
    const float val = init + e;
    cur[j] = val;
    if (j < S) {
      const size_t at = out + static_cast<size_t>(t0) * static_cast<size_t>(S) + static_cast<size_t>(j);
      float alpha = 0.0f;
      if constexpr (BWD) alpha = a.lat[at];
      emit_out<BWD>(a, at, val, e, alpha, total);
    }
  }
  wave_sync();
  float *last = cur;
  if (staged) wave_frames<K, TYPE, BWD, true>(a, rows, a.lat, out, total, T, S, ld, lane, arc0, col, prior, cur, nxt, em, ax, abeg, alp, asrc, &last);
  else wave_frames<K, TYPE, BWD, false>(a, rows, a.lat, out, total, T, S, ld, lane, arc0, col, prior, cur, nxt, em, ax, abeg, alp, asrc, &last);

  if constexpr (!BWD) {
    // the total: S <= 256, so partial i holds state i's term alone; a lane's slots are partials lane + 64 k
    const float ninf = float_of(kMinusInf);
    float p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = lane + k * kWaveLanes;
      p[k] = ninf;
      if (j < S) {
        const float term = last[j] + final_of(a.final_lp ? a.final_lp + s0 : nullptr, j, S);
        if (term == term) p[k] = ladd(p[k], term);
      }
    }
    p[0] = ladd(p[0], p[2]), p[1] = ladd(p[1], p[3]);  // step 128
    p[0] = ladd(p[0], p[1]);                            // step 64
#pragma unroll
    for (int step = 32; step >= 1; step /= 2) p[0] = ladd(p[0], __shfl_down(p[0], step));  // (lanes below `step` hold the tree's partials)
    if (lane == 0) a.total[L.total_off[seg]] = p[0];
  }
}

template <int TYPE, bool BWD>
__global__ __launch_bounds__(kWgThreads) void fb_wg_kernel(const Launch L, const Args a) {
  extern __shared__ uint32_t lds32[];
  const int seg = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x);
  const int T = L.T[seg], S = L.S[seg], ld = L.ld[seg], s0 = L.state0[seg], arc0 = L.arc0[seg], n_arcs = L.n_arcs[seg];
  const float *rows = a.rows + L.row_off[seg];
  const size_t out = static_cast<size_t>(L.out_off[seg]);
  float *cur = reinterpret_cast<float *>(lds32), *nxt = cur + L.d_floats, *red = nxt + L.d_floats;
  const float ninf = float_of(kMinusInf), nan = float_of(kQuietNaN);
  const float total = BWD ? a.total[L.total_off[seg]] : 0.0f;

  auto emit = [&](int t, int j) {
    const State st = load_state<TYPE>(a, s0 + j, true, ld);
    const float v = st.valid() ? rows[static_cast<size_t>(t) * static_cast<size_t>(ld) + static_cast<size_t>(st.col)] : nan;
    return align::emission(v, st.prior, a.floor, TYPE);
  };
  for (int u = 0; u < T; ++u) {
    const int t = BWD ? T - 1 - u : u;
    for (int j = tid; j < S; j += kWgThreads) {
      const float e = emit(t, j);  // (does not depend on d)
      const size_t at = out + static_cast<size_t>(t) * static_cast<size_t>(S) + static_cast<size_t>(j);
      float alpha = 0.0f;
      if constexpr (BWD) alpha = a.lat[at];
      float acc;
      if (u == 0) {
        acc = init_of<BWD>(a.init_lp ? a.init_lp + s0 : nullptr, j, S);
      } else {
        const int a0 = clampi(a.ptr[s0 + j] - arc0, 0, n_arcs), a1 = clampi(a.ptr[s0 + j + 1] - arc0, a0, n_arcs);
        acc = ninf;
        for (int i = a0; i < a1; ++i) {
          const int src = a.src[arc0 + i];
          acc = accumulate(acc, static_cast<unsigned>(src) < static_cast<unsigned>(S) ? cur[src] : nan, a.lp[arc0 + i]);
        }
      }
      const float val = acc + e;
      nxt[j] = val;
      emit_out<BWD>(a, at, val, e, alpha, total);
    }
    __syncthreads();
    float *sw = cur;
    cur = nxt, nxt = sw;
  }
  if constexpr (!BWD) {
    // the total: thread i owns partial i, its states in ascending order; then the tree, a barrier a step
    float p = ninf;
    for (int j = tid; j < S; j += kWgThreads) {
      const float term = cur[j] + final_of(a.final_lp ? a.final_lp + s0 : nullptr, j, S);
      if (term == term) p = ladd(p, term);
    }
    red[tid] = p;
    __syncthreads();
    for (int step = kPartials / 2; step >= 1; step /= 2) {
      if (tid < step) red[tid] = ladd(red[tid], red[tid + step]);
      __syncthreads();
    }
    if (tid == 0) a.total[L.total_off[seg]] = red[0];
  }
}

__global__ __launch_bounds__(256) void fb_math_kernel(int op, const float *x, const float *y, float *out, long long n) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) out[i] = op == 0 ? exp_neg(x[i]) : ladd(x[i], y[i]);
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
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * wg_lds_words(kMaxStates));
    attr_set.fetch_or(dev_bit, std::memory_order_release);
  }
  hipLaunchKernelGGL(kernel, dim3(l.n_segs), dim3(kWgThreads), l.lds_bytes, s, l, a);
}

template <int TYPE, bool BWD>
void launch_typed(const Launch &l, const Args &a, hipStream_t s) {
  const dim3 grid(l.n_segs);
  if (l.form == kWorkgroup) {
    launch_wg(fb_wg_kernel<TYPE, BWD>, l, a, s);
    return;
  }
  switch (l.K) {
    case 1: hipLaunchKernelGGL((fb_wave_kernel<1, TYPE, BWD>), grid, dim3(kWaveLanes), l.lds_bytes, s, l, a); break;
    case 2: hipLaunchKernelGGL((fb_wave_kernel<2, TYPE, BWD>), grid, dim3(kWaveLanes), l.lds_bytes, s, l, a); break;
    default: hipLaunchKernelGGL((fb_wave_kernel<4, TYPE, BWD>), grid, dim3(kWaveLanes), l.lds_bytes, s, l, a); break;
  }
}

template <bool BWD>
void launch_direction(const fb::Plan &p, const Args &a, int type, hipStream_t s) {
  for (const Launch &l : p.launches) {
    g_fb_launches.bump((BWD ? 2 : 0) + (l.form == kWave ? 0 : 1));
    if (type == kScores) launch_typed<kScores, BWD>(l, a, s);
    else if (type == loglik::kF16) launch_typed<loglik::kF16, BWD>(l, a, s);
    else launch_typed<loglik::kF32, BWD>(l, a, s);
  }
}

}  // namespace

void launch_fb(const fb::Plan &p, const FbArgs &g, hipStream_t s) {
  const bool want = g.d_gamma != nullptr;
  const Args f{g.d_rows, g.d_col, g.d_state_node, g.d_log_prior, g.width, g.floor, g.d_arc_ptr, g.d_arc_src, g.d_arc_lp, g.d_start_lp, g.d_final_lp,
               want ? g.d_scratch : nullptr, nullptr, g.d_total};
  launch_direction<false>(p, f, g.type, s);
  if (!want) return;
  const Args b{g.d_rows, g.d_col, g.d_state_node, g.d_log_prior, g.width, g.floor, g.d_t_ptr, g.d_t_src, g.d_t_lp, g.d_final_lp, nullptr,
               g.d_scratch, g.d_gamma, g.d_total};
  launch_direction<true>(p, b, g.type, s);
}

void launch_fb_math(int op, const float *d_a, const float *d_b, float *d_out, long long n, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(fb_math_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, op, d_a, d_b, d_out, n);
}

void fb_launch_counts(unsigned long long out[4]) { g_fb_launches.read(out); }
int fb_kernel_mode() { return g_fb_mode.load(std::memory_order_relaxed); }
void fb_kernel_mode(int mode) { g_fb_mode.store(mode, std::memory_order_relaxed); }

}  // namespace fdnn
