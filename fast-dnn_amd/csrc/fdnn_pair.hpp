// fdnn_pair.hpp -- pmaddubsw pair saturation (dnn.cc:337-340): the one definition of its arithmetic.
//
// The MFMA (or dot-product) sum of a node is exact; the reference saturates every ADJACENT pair
// a[2j]*w[2j] + a[2j+1]*w[2j+1] to int16.  Only the few (node, pair) entries listed at load time can saturate at all
// (fdnn_model.cpp).  A kernel recomputes such a pair from the staged s8 activation bytes and adds sat16(p) - p to the
// accumulator that holds (node, frame).  Two stored forms of the list:
//   * FixEntry words, 64 bits {u16 k, s8 w0, s8 w1, s32 node}, per 64-node group sorted by k: the GEMMs (fdnn_gemm.hip,
//     fdnn_chain.hip, fdnn_pp.hip, fdnn_ppo.hip, fdnn_small.hip) consume them as their k-loop brings the columns through
//     LDS.  A wave walks the entries of its 64 nodes with a FixCursor; when the k-step holding an entry's columns is in
//     LDS it screens the pair, and corrects where a frame fires.  The walk and the register select are wave-uniform; a
//     layer without risky pairs has k_next = INT_MAX.
//   * per-node 32-bit words k | w0 << 16 | w1 << 24 (fdnn_lists.hpp: build_node_fix_index): the kernels that score
//     single (row, node) pairs (fdnn_lists.hip, fdnn_set_tile.hpp).
// What stays in each kernel is its SCHEDULE: where in the k-loop it screens, which ring buffer it reads, its loops over
// frame blocks and its accumulator select.
//
// The 256-VGPR kernels sit on a register-allocation knife edge (profiles/LABBOOK.md, tools/kernel_resources.py): everything
// here is a plain aggregate without constructors, and a small helper that takes and returns BY VALUE.  The same helpers
// taking references, or a member initialiser in FixCursor, cost the chained kernel 79 .. 294 spilled registers.
//
// No HIP needed for the arithmetic: tests/host/pair_check.cpp builds this header alone with a host compiler.
#pragma once
#include <climits>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FDNN_PAIR_HD __host__ __device__ __forceinline__
#else
#define FDNN_PAIR_HD inline
#endif

namespace fdnn {

// ---- the two stored forms
struct PairEntry {
  int k, w0, w1, node;  // k: the pair's even column; node: FixEntry words only
};
FDNN_PAIR_HD int entry_k(uint64_t raw) { return static_cast<int>(raw & 0xffff); }
FDNN_PAIR_HD PairEntry decode_entry(uint64_t raw) {  // a FixEntry word
  return PairEntry{entry_k(raw), static_cast<int8_t>(raw >> 16), static_cast<int8_t>(raw >> 24), static_cast<int>(raw >> 32)};
}
FDNN_PAIR_HD PairEntry decode_pair(uint32_t raw) {  // a per-node word (lists::pack_pair)
  return PairEntry{static_cast<int>(raw & 0xffffu), static_cast<int8_t>(raw >> 16), static_cast<int8_t>(raw >> 24), 0};
}

// ---- the correction: sat16(p) - p for p = a0 * w0 + a1 * w1, from the pair's two staged bytes (s8 = u8 - 128, the
// 16-bit value read at the even column)
FDNN_PAIR_HD int pair_excess(uint32_t pair, int w0, int w1) {
  const int a0 = static_cast<int>((pair & 0xff) ^ 0x80), a1 = static_cast<int>((pair >> 8) ^ 0x80);  // back to u8
  const int prod = a0 * w0 + a1 * w1;
  return (prod > 32767 ? 32767 : prod < -32768 ? -32768 : prod) - prod;
}

// ---- the screen.  A pair that CAN saturate almost never does (both activations must be close to 255: 0.2 % of the
// (pair, frame) combinations of the Gaussian bench net, under 1 % of the pairs for any of a wave's 160 frames), so the
// common case only has to prove "no frame of this wave saturates": one frame per lane (not per half-wave as the
// accumulator layout has it), the pair as one 16-bit LDS read, the pair product as one v_dot4c_i32_i8 on the staged s8
// bytes (a = s8 + 128, so p = dot + 128 * (w0 + w1)), one range test.  Only when some lane fires does the wave run the
// exact correction.
struct PairScreen {
  int wpk, pbase;  // the weights as dot4 bytes 0 and 1; 128 * (w0 + w1) + 32768
};
FDNN_PAIR_HD PairScreen pair_screen(int w0, int w1) { return PairScreen{(w0 & 0xff) | ((w1 & 0xff) << 8), 128 * (w0 + w1) + 32768}; }
// v: the pair's 16-bit value.  True iff p leaves int16, i.e. iff pair_excess(v, w0, w1) != 0.
FDNN_PAIR_HD bool pair_fires(int v, PairScreen s) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int ps = __builtin_amdgcn_sdot4(v, s.wpk, s.pbase, false);  // p + 32768
#else
  int ps = s.pbase;
  for (int i = 0; i < 4; ++i) ps += static_cast<int8_t>(v >> (8 * i)) * static_cast<int8_t>(s.wpk >> (8 * i));
#endif
  return static_cast<unsigned>(ps) > 65535u;
}

// ---- where (node, frame) lives.  D layout of the 32 x 32 MFMA: column (frame) = lane & 31, row (node) =
// (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).  Node 0 .. 63 of a wave's two tiles is register idx = mi * 16 + reg of the
// lanes with lane >> 5 == half.
struct AccSlot {
  int idx, half;
};
FDNN_PAIR_HD AccSlot acc_slot(int node) {
  const int rr = node & 31;
  return AccSlot{(node >> 5) * 16 + (rr & 3) + 4 * (rr >> 3), (rr >> 2) & 1};
}

// ---- the cursor over a 64-node group's k-sorted FixEntry words.  Entries are walked with SCALAR loads (constant
// address space: s_load_dwordx2 into SGPRs, two entries ahead): no LDS round trip and no v_readfirstlane per entry, and
// the scalar cache path does not queue behind the LDS-DMA loads as a vector load issued in the loop would (-4.5 % on a
// Gaussian-weight layer against an LDS copy of the list).
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) uint64_t *FixPtr;
#else
typedef const uint64_t *FixPtr;
#endif
FDNN_PAIR_HD FixPtr fix_entries(const void *fix_ent) { return (FixPtr)(uintptr_t)fix_ent; }
FDNN_PAIR_HD int wave_uniform(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_readfirstlane(v);
#else
  return v;
#endif
}

struct FixCursor {  // closed: {0, 0, INT_MAX, ent, 0, 0}
  int e, end, k_next;     // the current entry, the group's end, the current entry's k (INT_MAX: none left)
  FixPtr ent;
  uint64_t raw, raw_nxt;  // entries e and e + 1
};
// the cursor at the first entry of group grp (fix_grp[grp] .. fix_grp[grp + 1])
FDNN_PAIR_HD FixCursor fix_open(FixCursor fx, const int32_t *fix_grp, int grp) {
  fx.e = wave_uniform(fix_grp[grp]);
  fx.end = wave_uniform(fix_grp[grp + 1]);
  if (fx.e < fx.end) {
    fx.raw = fx.ent[fx.e];
    if (fx.e + 1 < fx.end) fx.raw_nxt = fx.ent[fx.e + 1];
    fx.k_next = entry_k(fx.raw);
  }
  return fx;
}
FDNN_PAIR_HD FixCursor fix_advance(FixCursor fx) {
  ++fx.e;
  fx.raw = fx.raw_nxt;
  fx.k_next = fx.e < fx.end ? entry_k(fx.raw) : INT_MAX;
  if (fx.e + 1 < fx.end) fx.raw_nxt = fx.ent[fx.e + 1];
  return fx;
}

}  // namespace fdnn
