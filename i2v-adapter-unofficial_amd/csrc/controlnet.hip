// ControlNet residuals into the UNet's skip tensors (unet:1379-1403): i2v_add_residuals_f16.
//
//   out_i = skip_i + s * res_i,   s = scale_table[min(step_idx[0], rows - 1)]   (include/i2v_hip.h)
//
// for up to I2V_ADD_RES_MAX tensors of different sizes in ONE launch.  Memory-bound: 16 bytes per lane and access, AR_UNROLL
// independent accesses per lane in flight, at most AR_MAX_BLOCKS workgroups that stride over the tiles.  A tile is AR_TILE
// consecutive 16-byte chunks of ONE tensor; the tensor of a tile is found by a walk over the prefix sums of the tensors' tile
// counts, which travel with the pointers in the by-value parameter block (the kernarg segment): the launch reads no descriptor
// table from device memory, so a captured launch owns everything it reads except the operands, the scale table and the step counter.
// The walk is uniform over the workgroup (blockIdx only): pointers and bounds stay in scalar registers.
//
// dst may be skip (each lane reads its chunk before it writes it, and no other lane touches that chunk).  The scale comes from
// device memory so that a replayed graph can switch the control on and off over a schedule by its step counter.
//
// i2v_add_multi_residuals_f16 is the same launch for the residuals of up to I2V_ADD_RES_NETS_MAX ControlNets at once:
//
//   out_i = skip_i + sum_k s_k * res_k_i,   s_k = scale_table[k * rows + min(step_idx[0], rows - 1)]
//
// The skip is read once and written once whatever the number of nets: (N + 2) streams instead of the 3 N of N launches, and one
// rounding to fp16 instead of N.  One kernel per number of nets, so that a lane's loads -- (N + 1 or N + 2) * AM_UNROLL<N> of 16 bytes
// -- are all issued before the first is used; a tile stays 16 KB of each operand, walked in AR_UNROLL / AM_UNROLL<N> batches.
#include "common.h"
#include "residual_chunk.h"

namespace {

constexpr int AR_THREADS = 256;
constexpr int AR_UNROLL = 4;
constexpr int AR_TILE = AR_THREADS * AR_UNROLL;      // 16-byte chunks per tile: 16 KB of each operand
constexpr int AR_MAX_BLOCKS = 2048;

struct ArTensor {
  f16* dst;
  f16* dst_lo;
  const f16* skip;
  const f16* skip_lo;
  const f16* res;
  int64_t chunks;                                      // 16-byte chunks (8 values)
};

struct ArArgs {
  ArTensor t[I2V_ADD_RES_MAX];
  uint32_t tile_end[I2V_ADD_RES_MAX];                  // prefix sums of the tile counts: tiles of tensor i are [tile_end[i - 1], tile_end[i])
  int32_t n;
  int32_t scale_rows;
  const float* scale_table;
  const int32_t* step_idx;
};

// (one chunk: ar_chunk, residual_chunk.h -- shared with the T2I-Adapter's broadcast add)
template <bool HAS_LO>
__device__ __forceinline__ void ar_tile(const ArTensor& t, int64_t first, float s) {
  f16x8 hi[AR_UNROLL], lo[AR_UNROLL], r[AR_UNROLL];
#pragma unroll
  for (int u = 0; u < AR_UNROLL; ++u) {
    const int64_t c = first + u * AR_THREADS;
    if (c < t.chunks) {
      hi[u] = ld_global_16B(t.skip + c * 8);
      r[u] = ld_global_16B(t.res + c * 8);
      if (HAS_LO) lo[u] = ld_global_16B(t.skip_lo + c * 8);
    }
  }
#pragma unroll
  for (int u = 0; u < AR_UNROLL; ++u) {
    const int64_t c = first + u * AR_THREADS;
    if (c < t.chunks) {
      f16x8 o, ol;
      ar_chunk<HAS_LO>(hi[u], lo[u], r[u], s, o, ol);
      *reinterpret_cast<f16x8*>(t.dst + c * 8) = o;
      if (HAS_LO) *reinterpret_cast<f16x8*>(t.dst_lo + c * 8) = ol;
    }
  }
}

__global__ __launch_bounds__(AR_THREADS) void add_residuals_kernel(const ArArgs a) {
  float s = 1.0f;
  if (a.scale_table) {
    int row = a.step_idx ? a.step_idx[0] : 0;
    row = row < 0 ? 0 : (row > a.scale_rows - 1 ? a.scale_rows - 1 : row);
    s = a.scale_table[row];
  }
  const uint32_t tiles = a.tile_end[a.n - 1];
  int ti = 0;                                           // tiles only grow along the stride: the walk never restarts
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    while (tile >= a.tile_end[ti]) ++ti;                // ti < n: tile < tile_end[n - 1]
    const ArTensor& t = a.t[ti];
    const uint32_t begin = ti ? a.tile_end[ti - 1] : 0u;
    const int64_t first = (int64_t)(tile - begin) * AR_TILE + threadIdx.x;
    if (t.skip_lo)
      ar_tile<true>(t, first, s);
    else
      ar_tile<false>(t, first, s);
  }
}

// ---------------------------------------------------------------------------------------------- several nets
struct AmTensor {
  f16* dst;
  f16* dst_lo;
  const f16* skip;
  const f16* skip_lo;
  const f16* res[I2V_ADD_RES_NETS_MAX];
  int64_t chunks;
};

struct AmArgs {
  AmTensor t[I2V_ADD_RES_MAX];
  uint32_t tile_end[I2V_ADD_RES_MAX];
  int32_t n;
  int32_t scale_rows;
  const float* scale_table;                            // [nets, scale_rows]
  const int32_t* step_idx;
};
static_assert(sizeof(AmArgs) <= 4096, "AmArgs travels by value: the kernarg segment holds 4 KB");

// Accesses per operand that a lane issues per batch.  From the compiler's resource report ("Several ControlNets"):
// with four the 3- and 4-net kernels take 96 and 121 VGPRs (5 and 4 waves per SIMD); with two they take 69 and 79 (7 and 6 waves,
// the one-net kernel's 7) and a lane still has 8 to 12 loads of 16 bytes in flight, as many as the one-net kernel has with four.
template <int NETS> constexpr int AM_UNROLL = NETS <= 2 ? 4 : 2;

template <int NETS, bool HAS_LO>
__device__ __forceinline__ void am_tile(const AmTensor& t, int64_t first, const float (&s)[NETS]) {
  constexpr int U = AM_UNROLL<NETS>;
#pragma unroll 1
  for (int b = 0; b < AR_UNROLL; b += U) {
    f16x8 hi[U], lo[U], r[U][NETS];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t c = first + (b + u) * AR_THREADS;
      if (c < t.chunks) {
        hi[u] = ld_global_16B(t.skip + c * 8);
#pragma unroll
        for (int k = 0; k < NETS; ++k) r[u][k] = ld_global_16B(t.res[k] + c * 8);
        if (HAS_LO) lo[u] = ld_global_16B(t.skip_lo + c * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t c = first + (b + u) * AR_THREADS;
      if (c < t.chunks) {
        f16x8 o, ol;
        ar_multi_chunk<NETS, HAS_LO>(hi[u], lo[u], r[u], s, o, ol);
        *reinterpret_cast<f16x8*>(t.dst + c * 8) = o;
        if (HAS_LO) *reinterpret_cast<f16x8*>(t.dst_lo + c * 8) = ol;
      }
    }
  }
}

template <int NETS>
__global__ __launch_bounds__(AR_THREADS) void add_multi_residuals_kernel(const AmArgs a) {
  float s[NETS];
#pragma unroll
  for (int k = 0; k < NETS; ++k) s[k] = 1.0f;
  if (a.scale_table) {
    int row = a.step_idx ? a.step_idx[0] : 0;
    row = row < 0 ? 0 : (row > a.scale_rows - 1 ? a.scale_rows - 1 : row);
#pragma unroll
    for (int k = 0; k < NETS; ++k) s[k] = a.scale_table[(int64_t)k * a.scale_rows + row];
  }
  const uint32_t tiles = a.tile_end[a.n - 1];
  int ti = 0;
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    while (tile >= a.tile_end[ti]) ++ti;                // ti < n: tile < tile_end[n - 1]
    const AmTensor& t = a.t[ti];
    const uint32_t begin = ti ? a.tile_end[ti - 1] : 0u;
    const int64_t first = (int64_t)(tile - begin) * AR_TILE + threadIdx.x;
    if (t.skip_lo)
      am_tile<NETS, true>(t, first, s);
    else
      am_tile<NETS, false>(t, first, s);
  }
}

}  // namespace

extern "C" int i2v_add_multi_residuals_f16(const i2v_add_multi_residuals_params* p, i2v_stream_t stream) {
  I2V_CHECK_ARG(p != nullptr, "i2v_add_multi_residuals_f16: null params");
  I2V_CHECK_ARG(p->n >= 1 && p->n <= I2V_ADD_RES_MAX, "i2v_add_multi_residuals_f16: n %d outside 1..%d", p->n, I2V_ADD_RES_MAX);
  I2V_CHECK_ARG(p->n_nets >= 1 && p->n_nets <= I2V_ADD_RES_NETS_MAX, "i2v_add_multi_residuals_f16: n_nets %d outside 1..%d", p->n_nets,
                I2V_ADD_RES_NETS_MAX);
  I2V_CHECK_ARG(p->scale_table == nullptr || p->scale_rows >= 1, "i2v_add_multi_residuals_f16: a scale table of %d rows per net",
                p->scale_rows);
  I2V_CHECK_ARG((reinterpret_cast<uintptr_t>(p->scale_table) & 3) == 0 && (reinterpret_cast<uintptr_t>(p->step_idx) & 3) == 0,
                "i2v_add_multi_residuals_f16: scale_table / step_idx must be 4-byte aligned");
  AmArgs a;
  uint64_t tiles = 0;
  for (int i = 0; i < p->n; ++i) {
    const i2v_add_multi_residuals_entry& e = p->t[i];
    I2V_CHECK_ARG(e.dst && e.skip, "i2v_add_multi_residuals_f16: null pointer (dst / skip of tensor %d)", i);
    I2V_CHECK_ARG((e.skip_lo == nullptr) == (e.dst_lo == nullptr),
                  "i2v_add_multi_residuals_f16: skip_lo and dst_lo of tensor %d come together (a low half in means a low half out)", i);
    I2V_CHECK_ARG(e.numel > 0 && e.numel % 8 == 0, "i2v_add_multi_residuals_f16: tensor %d has %lld values, not a positive multiple of 8", i,
                  (long long)e.numel);
    I2V_CHECK_ARG(i2v_al16(e.dst) && i2v_al16(e.dst_lo) && i2v_al16(e.skip) && i2v_al16(e.skip_lo),
                  "i2v_add_multi_residuals_f16: the operands of tensor %d must be 16-byte aligned", i);
    I2V_CHECK_ARG(e.dst_lo == nullptr || e.dst_lo != e.dst, "i2v_add_multi_residuals_f16: dst and dst_lo of tensor %d are the same memory", i);
    a.t[i].dst = reinterpret_cast<f16*>(e.dst);
    a.t[i].dst_lo = reinterpret_cast<f16*>(e.dst_lo);
    a.t[i].skip = reinterpret_cast<const f16*>(e.skip);
    a.t[i].skip_lo = reinterpret_cast<const f16*>(e.skip_lo);
    for (int k = 0; k < I2V_ADD_RES_NETS_MAX; ++k) {
      if (k < p->n_nets) {
        I2V_CHECK_ARG(e.res[k] != nullptr, "i2v_add_multi_residuals_f16: null pointer (res[%d] of tensor %d)", k, i);
        I2V_CHECK_ARG(i2v_al16(e.res[k]), "i2v_add_multi_residuals_f16: the operands of tensor %d must be 16-byte aligned", i);
        I2V_CHECK_ARG(e.res[k] != e.dst && e.res[k] != e.dst_lo, "i2v_add_multi_residuals_f16: dst of tensor %d is its res[%d]", i, k);
      }
      a.t[i].res[k] = k < p->n_nets ? reinterpret_cast<const f16*>(e.res[k]) : nullptr;
    }
    a.t[i].chunks = e.numel / 8;
    tiles += (uint64_t)i2v_cdiv(a.t[i].chunks, AR_TILE);
    I2V_CHECK_ARG(tiles < ((uint64_t)1 << 31), "i2v_add_multi_residuals_f16: problem too large");
    a.tile_end[i] = (uint32_t)tiles;
  }
  for (int i = p->n; i < I2V_ADD_RES_MAX; ++i) {
    a.t[i] = AmTensor{nullptr, nullptr, nullptr, nullptr, {nullptr, nullptr, nullptr, nullptr}, 0};
    a.tile_end[i] = (uint32_t)tiles;
  }
  a.n = p->n;
  a.scale_rows = p->scale_rows;
  a.scale_table = p->scale_table;
  a.step_idx = p->step_idx;
  const dim3 grid((unsigned)(tiles < AR_MAX_BLOCKS ? tiles : AR_MAX_BLOCKS)), block(AR_THREADS);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (p->n_nets) {
    case 1: hipLaunchKernelGGL(add_multi_residuals_kernel<1>, grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL(add_multi_residuals_kernel<2>, grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL(add_multi_residuals_kernel<3>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(add_multi_residuals_kernel<4>, grid, block, 0, st, a); break;
  }
  return i2v_check_launch("i2v_add_multi_residuals_f16");
}

extern "C" int i2v_add_residuals_f16(const i2v_add_residuals_params* p, i2v_stream_t stream) {
  I2V_CHECK_ARG(p != nullptr, "i2v_add_residuals_f16: null params");
  I2V_CHECK_ARG(p->n >= 1 && p->n <= I2V_ADD_RES_MAX, "i2v_add_residuals_f16: n %d outside 1..%d", p->n, I2V_ADD_RES_MAX);
  I2V_CHECK_ARG(p->scale_table == nullptr || p->scale_rows >= 1, "i2v_add_residuals_f16: a scale table of %d rows", p->scale_rows);
  I2V_CHECK_ARG((reinterpret_cast<uintptr_t>(p->scale_table) & 3) == 0 && (reinterpret_cast<uintptr_t>(p->step_idx) & 3) == 0,
                "i2v_add_residuals_f16: scale_table / step_idx must be 4-byte aligned");
  ArArgs a;
  uint64_t tiles = 0;
  for (int i = 0; i < p->n; ++i) {
    const i2v_add_residuals_entry& e = p->t[i];
    I2V_CHECK_ARG(e.dst && e.skip && e.res, "i2v_add_residuals_f16: null pointer (dst / skip / res of tensor %d)", i);
    I2V_CHECK_ARG((e.skip_lo == nullptr) == (e.dst_lo == nullptr),
                  "i2v_add_residuals_f16: skip_lo and dst_lo of tensor %d come together (a low half in means a low half out)", i);
    I2V_CHECK_ARG(e.numel > 0 && e.numel % 8 == 0, "i2v_add_residuals_f16: tensor %d has %lld values, not a positive multiple of 8", i,
                  (long long)e.numel);
    I2V_CHECK_ARG(i2v_al16(e.dst) && i2v_al16(e.dst_lo) && i2v_al16(e.skip) && i2v_al16(e.skip_lo) && i2v_al16(e.res),
                  "i2v_add_residuals_f16: the operands of tensor %d must be 16-byte aligned", i);
    I2V_CHECK_ARG(e.dst_lo == nullptr || e.dst_lo != e.dst, "i2v_add_residuals_f16: dst and dst_lo of tensor %d are the same memory", i);
    a.t[i].dst = reinterpret_cast<f16*>(e.dst);
    a.t[i].dst_lo = reinterpret_cast<f16*>(e.dst_lo);
    a.t[i].skip = reinterpret_cast<const f16*>(e.skip);
    a.t[i].skip_lo = reinterpret_cast<const f16*>(e.skip_lo);
    a.t[i].res = reinterpret_cast<const f16*>(e.res);
    a.t[i].chunks = e.numel / 8;
    tiles += (uint64_t)i2v_cdiv(a.t[i].chunks, AR_TILE);
    I2V_CHECK_ARG(tiles < ((uint64_t)1 << 31), "i2v_add_residuals_f16: problem too large");
    a.tile_end[i] = (uint32_t)tiles;
  }
  for (int i = p->n; i < I2V_ADD_RES_MAX; ++i) {
    a.t[i] = ArTensor{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    a.tile_end[i] = (uint32_t)tiles;
  }
  a.n = p->n;
  a.scale_rows = p->scale_rows;
  a.scale_table = p->scale_table;
  a.step_idx = p->step_idx;
  const unsigned grid = (unsigned)(tiles < AR_MAX_BLOCKS ? tiles : AR_MAX_BLOCKS);
  hipLaunchKernelGGL(add_residuals_kernel, dim3(grid), dim3(AR_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
  return i2v_check_launch("i2v_add_residuals_f16");
}
