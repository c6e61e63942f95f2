// fdnn_tile.hpp -- the int8 GEMM tile shared by the per-layer kernel (fdnn_gemm.hip) and the chained hidden-layer
// kernel (fdnn_chain.hip), by the role-split kernels' rings (fdnn_pp.hip, fdnn_ppo.hip) and, for the pieces they have,
// by the split-K kernels (fdnn_small.hip, fdnn_set_tile.hpp).  It holds
//   * the tile geometry / LDS map (GemmCfg), the chunk swizzles, the fragment read and the 16-bit read of a pair;
//   * the RING pieces of the 256-node tile that can be written once without changing a kernel's instruction stream: the
//     accumulators' start values (acc_start), the LDS-DMA of the sigmoid table, the biases and 128 * sum(w)
//     (aux_table_piece, aux_words), the stage load of one 1-KiB piece (StageSrc, stage_voff, stage_load).
// What stays in each kernel is its SCHEDULE: where it issues the loads, its waits and barriers, its sched_barriers, the
// loop's alignment, its debug and timing switches -- and its ACCUMULATORS: the arrays are local to the kernel and the
// wave-uniform register select of the walk is written there.  Every helper takes and returns BY VALUE, and takes what the
// kernel has derived from the lane (its half, its row), not the lane: the kernel knows the lane's range, a helper compiled
// on its own does not, and the address arithmetic comes out in another order.  The walk's screen and corrections, a
// sub-step's fragment reads and the hidden tile's row store stay written out in each kernel: every by-value form tried
// changed the streams of the 256-VGPR kernels ("where the epilogue arithmetic and the ring live").
// Including it brings the pair-saturation arithmetic (fdnn_pair.hpp) along: every kernel built on this tile walks the
// saturating pairs; the epilogue's arithmetic is fdnn_act.hpp's (through fdnn_device.hpp).
#pragma once
#include "fdnn_device.hpp"
#include "fdnn_pair.hpp"

namespace fdnn {

// WM waves along the nodes (64 each): 4 = the 256-node tile of every large shape; 2 / 1 = the 128- / 64-node tiles of
// the smallest batches, where one workgroup's operand stream is what a launch waits for (see launch_qgemm).
template <int NF, int WN, int BK, int STAGES, int WM = 4>
struct GemmCfg {
  static constexpr int K_STEP = BK;                  // bytes of every row per stage
  static constexpr int G_BM = 64 * WM;               // nodes per workgroup tile
  static constexpr int NW = WM * WN;                 // waves
  static constexpr int THREADS = 64 * NW;
  static constexpr int FT = 32 * NF * WN;            // frames per workgroup tile
  static constexpr int RPI = 1024 / BK;              // rows per 1-KiB wave instruction
  static constexpr int LPR = BK / 16;                // lanes per row
  static constexpr int W_BYTES = G_BM * BK;
  static constexpr int A_BYTES = FT * BK;
  static constexpr int STAGE = W_BYTES + A_BYTES;
  static constexpr int W_SLABS = G_BM / RPI;
  static constexpr int A_SLABS = FT / RPI;
  static constexpr int MIN_LOADS = W_SLABS / NW + A_SLABS / NW;  // fewest loads any wave issues per stage
  // one wave issues NLD 1-KiB loads per stage: weight slabs wave, wave+NW, ... then activation slabs wave, wave+NW, ...
  static constexpr int NLD_W = W_SLABS / NW;
  static constexpr int NLD_A = (A_SLABS + NW - 1) / NW;
  static constexpr int NLD = NLD_W + NLD_A;
  // Behind the ring: the sigmoid table (3 KiB window) and this tile's 256 biases, both
  // LDS-DMA'd before the first stage so the epilogue starts without a load phase.  After the k-loop the ring is reused for the s8
  // output tile FT x (256+16) bytes (hidden layers) / the per-wave e tiles (output layer).
  static constexpr int TS = G_BM + 16;  // row stride of the s8 output tile: 16-byte aligned, rows 16 apart share a bank (2-way at worst)
  static constexpr int EPI = 8192 + FT * TS;
  static constexpr int FIX_OFF = STAGE * STAGES;
  static constexpr int AUX_OFF = FIX_OFF;  // table at +0, biases at +3072
  static constexpr int RING = AUX_OFF + 4096;
  static constexpr int LDS = RING > EPI ? RING : EPI;
  static_assert(EPI <= FIX_OFF, "the epilogue tile must not reach the table/biases");
  static_assert(W_SLABS % NW == 0, "weight slabs must split evenly over the waves");
  static_assert(LDS <= 160 * 1024, "LDS ring exceeds the CU");
};

template <int BK>
__device__ __forceinline__ int swz(int row) {
  return BK == 64 ? ((row >> 2) & 3) : ((row >> 1) & 7);
}

template <int BK>
__device__ __forceinline__ v4i read_frag(const char *tile, int row, int chunk) {
  return *reinterpret_cast<const v4i *>(tile + row * BK + ((chunk ^ swz<BK>(row)) << 4));
}

// the two staged s8 bytes at columns kl, kl + 1 (kl even) of a tile row: what fdnn_pair.hpp's pair_fires / pair_excess take
template <int BK>
__device__ __forceinline__ uint32_t pair_at(const char *tile, int row, int kl) {
  return *reinterpret_cast<const uint16_t *>(tile + row * BK + (((kl >> 4) ^ swz<BK>(row)) << 4) + (kl & 15));
}

// The split-K kernels' images (fdnn_small.hip, fdnn_set_tile.hpp) have 256-byte rows: chunk c (16 bytes) of row r lives
// at chunk position c ^ (r & 15) -- the 16 lanes of a ds_read_b128 group read 16 different rows at the same k and land on
// 16 different 16-byte slots.
[[maybe_unused]] __device__ __forceinline__ int row256_pos(int row, int chunk) { return (row << 8) + (((chunk ^ row) & 15) << 4); }

#if defined(__HIP_DEVICE_COMPILE__)  // (buffer-resource builtins are device-only)

// ---- the accumulators' start values: 128 * sum_k(w[node][k]) (the s8 = u8 - 128 activation offset), so that the epilogue
// has no per-output add left.  D layout (32x32): column (frame) = lane&31, row (node) = (reg&3) + 8*(reg>>2) + 4*(lane>>5):
// registers 4g .. 4g + 3 of tile a of wave wm, the same for every frame block.
__device__ __forceinline__ int4 acc_start(const int32_t *wsum, int m0, int wm, int half, int a, int g) {
  return *reinterpret_cast<const int4 *>(wsum + m0 + 64 * wm + 32 * a + 8 * g + 4 * half);
}

// ---- L2 -> LDS.  Buffer loads (buffer_load_dwordx4 ... offen lds) with one descriptor per operand tile, ONE per-lane
// VGPR offset (row-in-slab * stride + swizzled chunk) and a scalar offset for slab + k-step.
struct StageSrc {
  __amdgpu_buffer_rsrc_t w, a;  // the tile's weight rows, its activation rows
  int voff_w, voff_a;           // the lane's offsets
  int ldw, lda;                 // the row strides
};
// the lane's part of a staging address: row = slab*RPI + lane/LPR, chunk swizzled by the row (for 128-byte rows the swizzle
// depends on the slab's parity = wave&1, because every wave takes slabs wave, wave+NW, ... and NW is even; a one-wave
// workgroup takes EVERY slab: the parity then alternates with the slab index, see stage_load)
template <class Cfg>
__device__ __forceinline__ int stage_voff(int lane, int wave, int ld) {
  static_assert(Cfg::NW % 2 == 0 || Cfg::NW == 1, "slab parity per wave needs an even wave count (or one wave)");
  const int srow = lane / Cfg::LPR;
  const int schunk = ((lane % Cfg::LPR) ^ swz<Cfg::K_STEP>(wave * Cfg::RPI + srow)) << 4;
  return srow * ld + schunk;
}
// piece i (0 .. NLD - 1) of this wave's share of stage kt into ring buffer buf.  A_AUX: the cache policy of the
// activation rows' loads (the weights' is the default).
template <class Cfg, int A_AUX = 0>
__device__ __forceinline__ void stage_load(char *smem, StageSrc src, int wave, int kt, int buf, int i) {
  constexpr int NW = Cfg::NW, BK = Cfg::K_STEP;
  char *base = smem + buf * Cfg::STAGE;
  const int koff = kt * BK;
  // swz<128>(8 * slab + srow) = (4 * slab + (srow >> 1)) & 7: an odd slab flips chunk bit 2 = offset bit 6 (the row
  // strides are multiples of 128 bytes, so the flip stays inside the chunk field)
  const int odd = (NW == 1 && BK == 128) ? 64 : 0;
  if (i < Cfg::NLD_W) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(src.w, FDNN_LDS_PTR(base + (i * NW + wave) * 1024), 16, (i & 1) ? src.voff_w ^ odd : src.voff_w,
                                             (i * NW + wave) * Cfg::RPI * src.ldw + koff, 0, 0);
  } else {
    const int s = i - Cfg::NLD_W;
    if (Cfg::A_SLABS % NW == 0 || s * NW + wave < Cfg::A_SLABS)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(src.a, FDNN_LDS_PTR(base + Cfg::W_BYTES + (s * NW + wave) * 1024), 16,
                                               (s & 1) ? src.voff_a ^ odd : src.voff_a, (s * NW + wave) * Cfg::RPI * src.lda + koff, 0, A_AUX);
  }
}

// ---- the epilogue's sigmoid table and biases ride the LDS-DMA queue ahead of the ring (older loads complete first, so
// every wait that covers stage 0 covers them too).  The table goes as 1-KiB pieces (three cover it), one wave each.
// The range of a 16-byte LDS-DMA access is checked as a whole: with num_records = the table
// size, the lane holding the table's last three (half-step) / last one (exact) entries read zeros --
// u8 128 instead of 255 for every activation with lin >= 6.395 (found by
// test_net_with_every_pair_saturating; rare on trained nets, never on the round-1 fixtures).
// The blob pads both tables to 16 bytes (fdnn_model.cpp: place(size + 15)): table_bytes = (size + 15) & ~15.
__device__ __forceinline__ void aux_table_piece(char *aux, const uint8_t *table, int table_bytes, int piece, int lane) {
  const __amdgpu_buffer_rsrc_t rsrc_lut = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(table), 0, table_bytes, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_lut, FDNN_LDS_PTR(aux + piece * 1024), 16, lane * 16, piece * 1024, 0, 0);
}
// n 32-bit words -- a tile's biases, its 128 * sum(w) -- to dst (n * 4 <= 1024: one wave's load; lanes past them read nothing)
__device__ __forceinline__ void aux_words(char *dst, const void *src, int n, int lane) {
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(src), 0, n * 4, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, FDNN_LDS_PTR(dst), 16, lane * 16, 0, 0, 0);
}

#endif  // __HIP_DEVICE_COMPILE__

}  // namespace fdnn
