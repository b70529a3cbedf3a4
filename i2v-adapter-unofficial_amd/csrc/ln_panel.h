// The LayerNorm panel of the persistent fused kernels (ln_qkv.hip, ff_fused.hip, motion_attn.hip): ONE definition of its LDS format
// and of every scheduling fact around it.
//
// A workgroup of 8 waves owns a tile of 16 PIX rows (PIX 16-row MFMA tiles; 128 rows at C = 320, 64 at C = 640: 80 KB either way).
// A wave fetches its RW = 16 PIX / 8 rows RAW by LDS-DMA into its own slice of a panel (RW x C halfs at row RW wave, in
// [group of 8 rows][64-channel column][lane] order: one DMA instruction moves 8 rows x 128 bytes) and LayerNorms them: read whole
// into registers, then written to their places in the panel's format
//     row r at r C halfs, its 16-byte chunk c at position c ^ (r & 7)
// so that the 16 rows of a fragment read land on distinct banks.  No register holds a row while the DMA is in flight under the
// previous tile's last pass (held in registers there, they spilled: 259 dwords, 121 -> 230 us for motion_attn).  Then a
// software-pipelined K loop (`panel_project`) runs weight fragments, streamed from L2 in fragment order, against the panel.
// What differs between the kernels -- what runs under the DMA, the accumulators' epilogues, the tile loops -- stays in their files.
#pragma once

#include <type_traits>

#include "common.h"

// buffer_load_dwordx4 ... offen lds: 16 bytes per lane, global -> LDS at (wave-uniform LDS base) + 16 * lane (a plain function
// on purpose, as in gemm_big.hip: called directly from the kernel template, the builtin makes hipcc drop the launch stub)
__device__ __forceinline__ void panel_dma16(__amdgpu_buffer_rsrc_t rsrc, f16* lds_wave_base, unsigned voff, unsigned soff = 0) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds_wave_base, 16, voff, soff, 0, 0);
}
// a copy of a lane-dependent value that the compiler cannot see through: address arithmetic derived from it is redone where it is
// used instead of being hoisted out of the tile loop as a loop invariant.  (r5: hoisted, the ten DMA offsets of `panel_fetch_rows`
// and the output rows' store addresses of a tile were SPILLED, and every reload was followed by `s_waitcnt vmcnt(0)` -- scratch
// loads count on vmcnt -- so each DMA instruction waited for the one before it to land and each store for the weight fragments in
// flight: ten HBM round trips in series per tile.)
__device__ __forceinline__ int panel_opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

constexpr int PANEL_PD = 3;            // weight fragment sets of `panel_project`: the one in use and two K steps ahead
constexpr int PANEL_AD = 4;            // panel fragments in flight (reads ahead of the MFMAs that take them)

// The wave's RW raw rows from `base` (wave-uniform: the first of them) into its slice of a panel.  No wait: the caller knows what
// else is in flight (loads return in order).
template <int C, int RW>
__device__ __forceinline__ void panel_fetch_rows(const f16* base, const int64_t ldx, f16* slice, const int lane) {
  constexpr int NJ = C / 64;
  static_assert(C % 64 == 0 && RW % 8 == 0, "8 lanes x C / 64 chunks per row, whole groups of 8 rows per wave");
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(base), 0, (int)(((RW - 1) * ldx + C) * 2), 0x00020000);
  const int ln = panel_opaque(lane);
  const unsigned voff = (unsigned)(((ln >> 3) * ldx + (ln & 7) * 8) * 2);      // the instruction's part is a scalar offset
#pragma unroll
  for (int half = 0; half < RW / 8; ++half)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      panel_dma16(rs, slice + (half * NJ + j) * 512, voff, (unsigned)((8 * half * ldx + 8 * j * 8) * 2));
}

// `row_table` of `panel_normalise_rows` for a second table that is one row of C values (LayerNorm's beta): read once, ahead of
// the rows
struct panel_one_table {
  __device__ __forceinline__ const float* operator()(const float* table, const int) const { return table; }
};

// The wave's RW raw rows (`raw`: its slice as `panel_fetch_rows` filled it, landed) normalised into rows row0 .. row0 + RW - 1 of
// `panel`: (x - mean) rstd * gamma + second table, 8 lanes per row.  `raw` may be the same rows of `panel` (in place: every lane
// has read all its values before the first write).  gamma and the second table are fp32 (no conversions, one add less where the
// caller folds a positional table into beta).  `row_table(t, row)`: the second table's row for panel row `row` -- it receives
// the LAUNDERED base pointer t, and must derive the row's address from that one (from the original pointer, one motion_attn
// instantiation went from 0 to 40 bytes of scratch and another from 219 to 245 registers).
template <int C, int RW, class RowTable>
__device__ __forceinline__ void panel_normalise_rows(const f16* raw, f16* panel, const int row0, const int lane, const float* gamma,
                                                     const float* second, const float eps, RowTable row_table) {
  constexpr int NJ = C / 64, HALVES = RW / 8;
  constexpr bool ONCE = std::is_same<RowTable, panel_one_table>::value;
  // (NJ > 5, the C = 640 form: a row's slice is 80 values per lane, and gamma, the second table's row and the values together would
  // be 240 registers -- there the two tables are read per 64-channel column where they are applied instead of ahead of the row's sums)
  constexpr bool LATE_TABLES = NJ > 5;
  const int sub = lane & 7;
  f16x8 xv[HALVES][NJ];
#pragma unroll
  for (int half = 0; half < HALVES; ++half)
#pragma unroll
    for (int j = 0; j < NJ; ++j) xv[half][j] = *reinterpret_cast<const f16x8*>(raw + ((half * NJ + j) * 64 + lane) * 8);
  // (the tables are loop invariants: without the opaque copies of their addresses the compiler keeps all 80 - 120 registers of
  // them live through the passes of every tile -- 207 spilled dwords in motion_attn)
  const float* gp = gamma;
  const float* sp = second;
  asm volatile("" : "+s"(gp), "+s"(sp));
  f32x4 ga[NJ][2], sv[NJ][2];
  if constexpr (!LATE_TABLES) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      ga[j][0] = *reinterpret_cast<const f32x4*>(gp + (sub + 8 * j) * 8);
      ga[j][1] = *reinterpret_cast<const f32x4*>(gp + (sub + 8 * j) * 8 + 4);
      if constexpr (ONCE) {
        sv[j][0] = *reinterpret_cast<const f32x4*>(sp + (sub + 8 * j) * 8);
        sv[j][1] = *reinterpret_cast<const f32x4*>(sp + (sub + 8 * j) * 8 + 4);
      }
    }
  }
#pragma unroll
  for (int half = 0; half < HALVES; ++half) {
    const int row = row0 + 8 * half + (lane >> 3);
    const float* sh = row_table(sp, row);      // (read where the second table is per row or the tables are late; ONCE: sv is loaded)
    if constexpr (!LATE_TABLES && !ONCE) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        sv[j][0] = *reinterpret_cast<const f32x4*>(sh + (sub + 8 * j) * 8);
        sv[j][1] = *reinterpret_cast<const f32x4*>(sh + (sub + 8 * j) * 8 + 4);
      }
    }
    float v[NJ][8];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[j][e] = (float)xv[half][j][e];
        s += v[j][e];
      }
    s = sum_lanes8(s);
    const float mean = s / (float)C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[j][e] -= mean;
        q = fmaf(v[j][e], v[j][e], q);
      }
    q = sum_lanes8(q);
    const float rstd = rsqrtf(q / (float)C + eps);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int ch = sub + 8 * j;
      if constexpr (LATE_TABLES) {
        ga[j][0] = *reinterpret_cast<const f32x4*>(gp + ch * 8);
        ga[j][1] = *reinterpret_cast<const f32x4*>(gp + ch * 8 + 4);
        sv[j][0] = *reinterpret_cast<const f32x4*>(sh + ch * 8);
        sv[j][1] = *reinterpret_cast<const f32x4*>(sh + ch * 8 + 4);
      }
      f16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (f16)fmaf(v[j][e] * rstd, ga[j][e >> 2][e & 3], sv[j][e >> 2][e & 3]);
      *reinterpret_cast<f16x8*>(panel + row * C + ((ch ^ (row & 7)) * 8)) = o;
    }
  }
}

// A lane's two offsets (halfs) into a panel row for MFMA fragment reads: lane (g = lane >> 4, l15 = lane & 15) takes chunk 4 s + g
// of row 16 pix + l15 in K step s.  Swizzled by the row, ((4 s + g) ^ sw) = 8 (s >> 1) + ((4 (s & 1) + g) ^ sw) with sw = l15 & 7:
// TWO lane-dependent offsets and an immediate, not one precomputed register per K step (those ten were hoisted out of the tile
// loop and spilled).
__device__ __forceinline__ void panel_fragment_offsets(const int lane, int (&swz)[2]) {
  const int g = lane >> 4, sw = lane & 7;
  swz[0] = (g ^ sw) * 8;
  swz[1] = ((4 + g) ^ sw) * 8;
}

// fragment i = s PIX + pix of a pass over the panel: K step s of 16-row tile pix (alane = panel + (lane & 15) C)
template <int C, int PIX>
__device__ __forceinline__ f16x8 panel_lda(const f16* alane, const int (&swz)[2], const int i) {
  return *reinterpret_cast<const f16x8*>(alane + 16 * (i % PIX) * C + 64 * ((i / PIX) >> 1) + swz[(i / PIX) & 1]);
}

// One pass over a panel: acc(pix, t) += panel tile pix x weight tile t over the C / 32 K steps, pix = 0 .. PIX - 1, t = 0 .. NT - 1.
//   ldw(s, t): the f16x8 weight fragment of K step s and tile t (a buffer load: lane offset in ONE register, the fragment's place
//     in the scalar offset -- as flat loads the fragment addresses of a tile are loop invariants that the compiler hoists as 64-bit
//     pairs: 180 registers, spilled); requested PANEL_PD - 1 K steps ahead of the MFMAs that take it
//   acc(pix, t): reference to the f32x4 accumulator; initialised by the caller
//   TR: the weight fragment is the A operand (D[weight row][panel row]); else the panel fragment is (D[panel row][weight row])
//   FENCE: a scheduling fence behind the first weight requests (r5: without it the scheduler may pair each of these loads with the
//     first MFMA that takes it -- load, s_waitcnt vmcnt(0), MFMA, three L2 round trips in series at the top of the pass: seen in the
//     v pass of motion_attn's out-projection form)
//   hook(s): called at the top of K step s behind that step's weight requests -- the place for memory requests that may return
//     behind the fragments requested so far (loads return in order)
template <int C, int PIX, int NT, bool TR, bool FENCE, class Ldw, class Acc, class Hook>
__device__ __forceinline__ void panel_project(const f16* panel, const int (&swz)[2], const int lane, Ldw ldw, Acc acc, Hook hook) {
  constexpr int KS = C / 32, NI = KS * PIX, PD = PANEL_PD, AD = PANEL_AD;
  const f16* alane = panel + (lane & 15) * C;
  f16x8 wf[PD][NT];
#pragma unroll
  for (int s = 0; s < PD - 1; ++s)
#pragma unroll
    for (int t = 0; t < NT; ++t) wf[s][t] = ldw(s, t);
  if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
  f16x8 af[AD + 1];
#pragma unroll
  for (int i = 0; i < AD; ++i) af[i] = panel_lda<C, PIX>(alane, swz, i);
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int s = i / PIX, pix = i % PIX;
    if (pix == 0 && s + PD - 1 < KS) {
#pragma unroll
      for (int t = 0; t < NT; ++t) wf[(s + PD - 1) % PD][t] = ldw(s + PD - 1, t);
    }
    if (pix == 0) hook(s);
    if (i + AD < NI) af[(i + AD) % (AD + 1)] = panel_lda<C, PIX>(alane, swz, i + AD);
#pragma unroll
    for (int t = 0; t < NT; ++t)
      acc(pix, t) = TR ? mfma16x16x32(wf[s % PD][t], af[i % (AD + 1)], acc(pix, t))
                       : mfma16x16x32(af[i % (AD + 1)], wf[s % PD][t], acc(pix, t));
    __builtin_amdgcn_sched_barrier(0);      // (unfenced, the scheduler hoists every load of the pass to its top: 947 spills)
  }
}
