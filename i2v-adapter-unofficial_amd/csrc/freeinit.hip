// FreeInit (https://arxiv.org/abs/2312.07537; diffusers FreeInitMixin._apply_free_init): the previous round's clean latents are
// diffused back to the initial noise level with the round-0 noise, and only their low spatio-temporal frequencies are kept; the high
// ones come from a fresh draw.  Per (b, c) volume over (F, H, W) of latents [B, F, C, H, W] fp32:
//
//   z_t = sa * latents + sb * init_noise
//   out = Re ifftn( ifftshift( fftshift(fftn(z_t)) * lpf + fftshift(fftn(z_rand)) * (1 - lpf) ) )
//       = z_rand + Re ifftn( ifftshift(lpf) * fftn(z_t - z_rand) )                  (linearity: one transform pair instead of three)
//
// with lpf [F, H, W] in the centred layout (index (t, h, w) = frequency (t - F/2, h - H/2, w - W/2)).  At an odd size the centred
// table is not symmetric about the zero frequency, the filtered spectrum is not Hermitian and the discarded imaginary part is not
// zero: the inverse below is a full complex one whose real part is taken at the very end.
//
// No FFT: F <= 32, H, W <= 128 and any length (96, 40, odd ones) must work, so every axis is a direct DFT, X[k] = sum_n x[n] T[(k n) mod N],
// with T an N-entry twiddle table per workgroup in LDS (sincospi in double, rounded once) indexed by an INTEGER (k n) mod N kept
// incrementally -- never an fp32 product of k and n.  Five launches of one kernel template, the complex volume living in a
// caller-owned workspace of B F C H W float2 laid out like the latents:
//
//   1. rows (W):  d = fma(sa, latents, sb * init_noise) - z_rand formed on load, forward DFT along W          -> workspace
//   2. columns (H): forward DFT along H, in place
//   3. frames (F):  forward DFT along F, times lpf at the shifted index, inverse DFT along F, in place (both in LDS)
//   4. columns (H): inverse DFT along H, in place
//   5. rows (W):  inverse DFT along W (real part only), out = z_rand + re / (F H W)
//
// A workgroup (256 threads) owns a tile of LT lines of one axis -- LT = 64 / 32 / 16 for N <= 32 / 64 / 128, so a tile is at most
// 2048 complex values -- stages it in LDS as [n][LT + 1] float2 (lanes along the line index: 8-byte reads without bank conflicts; the
// odd row stride keeps the transposing accesses of the row passes conflict-free too), and thread (line l, group kg) accumulates the
// 8 outputs k = kg + j * (256 / LT) in registers while it walks n once.  Results go through a second LDS tile so that every global
// access is coalesced along the memory-contiguous index.  In-place passes are safe: a tile is read whole before any of it is written,
// and tiles are disjoint.  LDS: 2 x 2176 float2 + 128 float2 twiddles + per-line tables = 36.7 KB, four workgroups per CU.
#include "common.h"

namespace {

constexpr int FI_THREADS = 256;
constexpr int FI_MAX_F = 32;
constexpr int FI_MAX_HW = 128;
constexpr int FI_KPT = 8;                  // outputs per thread: ceil(N / (FI_THREADS / LT)) <= 8 for every (N, LT) pair used
constexpr int FI_TILE = 2176;              // float2 per LDS tile: max over LT of N_max(LT) * (LT + 1) = 128 * 17
constexpr int64_t FI_MAX_ELEMS = (int64_t)1 << 30;

enum fi_mode { FI_ROWS_FWD = 0, FI_AXIS_FWD = 1, FI_FRAMES = 2, FI_AXIS_INV = 3, FI_ROWS_INV = 4 };

struct fi_args {
  const float* lat;        // FI_ROWS_FWD
  const float* noise;      // FI_ROWS_FWD
  const float* zr;         // FI_ROWS_FWD, FI_ROWS_INV
  const float* lpf;        // FI_FRAMES
  float* out;              // FI_ROWS_INV
  float2* ws;
  int64_t nlines;          // lines of this pass's axis
  int n;                   // length of the axis
  int64_t inner;           // stride of the axis in elements (1 for the row passes)
  int hh, ww;              // FI_FRAMES: the plane, for the filter's shifted index
  float sa, sb, scale;
};

// acc[j] = sum_n src[n][l] * (cos, sgn sin)(2 pi (k_j n mod N) / N), k_j = kg + j * KG; a k_j >= N walks entry 0 and is never stored;
// REAL_ONLY leaves acc[j].y at 0
template <int LT, bool FWD, bool REAL_ONLY = false>
__device__ __forceinline__ void fi_dft(const float2* __restrict__ src, const float2* __restrict__ tw, int n_len, int l, int kg,
                                       float2 (&acc)[FI_KPT]) {
  constexpr int KG = FI_THREADS / LT, LS = LT + 1;
  int kk[FI_KPT], idx[FI_KPT];
#pragma unroll
  for (int j = 0; j < FI_KPT; ++j) {
    const int k = kg + j * KG;
    kk[j] = k < n_len ? k : 0;
    idx[j] = 0;
    acc[j] = make_float2(0.f, 0.f);
  }
  for (int n = 0; n < n_len; ++n) {
    const float2 x = src[n * LS + l];
#pragma unroll
    for (int j = 0; j < FI_KPT; ++j) {
      const float2 t = tw[idx[j]];
      const float sn = FWD ? -t.y : t.y;
      acc[j].x = fmaf(x.x, t.x, acc[j].x);
      acc[j].x = fmaf(-x.y, sn, acc[j].x);
      if constexpr (!REAL_ONLY) {
        acc[j].y = fmaf(x.y, t.x, acc[j].y);
        acc[j].y = fmaf(x.x, sn, acc[j].y);
      }
      idx[j] += kk[j];                        // (k n) mod N, exact
      if (idx[j] >= n_len) idx[j] -= n_len;
    }
  }
}

template <int LT, int MODE>
__global__ __launch_bounds__(FI_THREADS) void freeinit_kernel(const fi_args a) {
  constexpr int KG = FI_THREADS / LT, LS = LT + 1;
  constexpr bool ROWS = MODE == FI_ROWS_FWD || MODE == FI_ROWS_INV;
  __shared__ float2 buf_a[FI_TILE], buf_b[FI_TILE], tw[FI_MAX_HW];
  __shared__ int64_t line_base[LT];
  __shared__ int line_lpf[LT];
  const int tid = threadIdx.x, n_len = a.n;
  const int64_t line0 = (int64_t)blockIdx.x * LT;
  const int lines = (int)(a.nlines - line0 < LT ? a.nlines - line0 : LT);      // >= 1: the grid is cdiv(nlines, LT)

  if (tid < n_len) {
    double s, c;
    sincospi(2.0 * (double)tid / (double)n_len, &s, &c);
    tw[tid] = make_float2((float)c, (float)s);
  }
  if (tid < lines) {
    const int64_t line = line0 + tid, o = line / a.inner, i = line - o * a.inner;
    line_base[tid] = o * n_len * a.inner + i;
    if constexpr (MODE == FI_FRAMES) {      // i = c H W + h W + w; the centred table's index of frequency (h, w) is ((h + H/2) % H, ...)
      const int r = (int)(i % ((int64_t)a.hh * a.ww)), hk = r / a.ww, wk = r - hk * a.ww;
      line_lpf[tid] = ((hk + a.hh / 2) % a.hh) * a.ww + (wk + a.ww / 2) % a.ww;
    }
  }
  __syncthreads();

  // ---- load the tile: buf_a[n][l].  Row passes: a tile is `lines * N` contiguous values; otherwise lanes run along the line index.
  const int total = lines * n_len;
  for (int e = tid; e < total; e += FI_THREADS) {
    int l, n;
    if constexpr (ROWS) { l = e / n_len; n = e - l * n_len; } else { n = e / lines; l = e - n * lines; }
    const int64_t g = line_base[l] + (int64_t)n * a.inner;
    float2 v;
    if constexpr (MODE == FI_ROWS_FWD)
      v = make_float2(fmaf(a.sa, a.lat[g], a.sb * a.noise[g]) - a.zr[g], 0.f);
    else
      v = a.ws[g];
    buf_a[n * LS + l] = v;
  }
  __syncthreads();

  const int l = tid % LT, kg = tid / LT;
  const bool live = l < lines && kg < n_len;
  float2 acc[FI_KPT];
  if (live) {
    if constexpr (MODE == FI_ROWS_FWD || MODE == FI_AXIS_FWD || MODE == FI_FRAMES)
      fi_dft<LT, true>(buf_a, tw, n_len, l, kg, acc);
    else      // (the last pass keeps the real part only: its imaginary sums are never formed)
      fi_dft<LT, false, MODE == FI_ROWS_INV>(buf_a, tw, n_len, l, kg, acc);
    if constexpr (MODE == FI_FRAMES) {
      const int64_t plane = (int64_t)a.hh * a.ww;
#pragma unroll
      for (int j = 0; j < FI_KPT; ++j) {
        const int k = kg + j * KG;
        if (k < n_len) {
          const float g = a.lpf[(int64_t)((k + n_len / 2) % n_len) * plane + line_lpf[l]];
          acc[j].x *= g;
          acc[j].y *= g;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < FI_KPT; ++j) {
      const int k = kg + j * KG;
      if (k < n_len) buf_b[k * LS + l] = acc[j];
    }
  }
  __syncthreads();
  const float2* res = buf_b;
  if constexpr (MODE == FI_FRAMES) {      // back along F from buf_b into buf_a (every forward read of buf_a is behind the barrier)
    if (live) {
      fi_dft<LT, false>(buf_b, tw, n_len, l, kg, acc);
#pragma unroll
      for (int j = 0; j < FI_KPT; ++j) {
        const int k = kg + j * KG;
        if (k < n_len) buf_a[k * LS + l] = acc[j];
      }
    }
    __syncthreads();
    res = buf_a;
  }

  // ---- store the tile, same index walk as the load
  for (int e = tid; e < total; e += FI_THREADS) {
    int sl, k;
    if constexpr (ROWS) { sl = e / n_len; k = e - sl * n_len; } else { k = e / lines; sl = e - k * lines; }
    const int64_t g = line_base[sl] + (int64_t)k * a.inner;
    const float2 v = res[k * LS + sl];
    if constexpr (MODE == FI_ROWS_INV)
      a.out[g] = fmaf(v.x, a.scale, a.zr[g]);
    else
      a.ws[g] = v;
  }
}

template <int MODE>
void fi_launch(const fi_args& a, hipStream_t st) {
  if (a.n <= 32)
    hipLaunchKernelGGL((freeinit_kernel<64, MODE>), dim3((unsigned)i2v_cdiv(a.nlines, 64)), dim3(FI_THREADS), 0, st, a);
  else if (a.n <= 64)
    hipLaunchKernelGGL((freeinit_kernel<32, MODE>), dim3((unsigned)i2v_cdiv(a.nlines, 32)), dim3(FI_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL((freeinit_kernel<16, MODE>), dim3((unsigned)i2v_cdiv(a.nlines, 16)), dim3(FI_THREADS), 0, st, a);
}

// the sizes the kernels take (b c first: the full product then stays far inside int64)
bool fi_sizes_ok(int32_t b, int32_t f, int32_t c, int32_t h, int32_t w) {
  return b > 0 && f > 0 && c > 0 && h > 0 && w > 0 && f <= FI_MAX_F && h <= FI_MAX_HW && w <= FI_MAX_HW &&
         (int64_t)b * c <= FI_MAX_ELEMS && (int64_t)b * c * f * h * w <= FI_MAX_ELEMS;
}

bool fi_overlap(const void* p, int64_t pb, const void* q, int64_t qb) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)qb && b < a + (uintptr_t)pb;
}

}  // namespace

extern "C" int64_t i2v_freeinit_workspace_bytes(int32_t b, int32_t f, int32_t c, int32_t h, int32_t w) {
  I2V_CHECK_ARG(fi_sizes_ok(b, f, c, h, w),
                "i2v_freeinit_workspace_bytes: not implemented for this problem (b %d f %d c %d h %d w %d: f in 1..%d, h and w in 1..%d, "
                "at most 2^30 values)", b, f, c, h, w, FI_MAX_F, FI_MAX_HW);
  return (int64_t)b * f * c * h * w * (int64_t)sizeof(float2);
}

extern "C" int i2v_freeinit_mix(const float* latents, const float* init_noise, const float* z_rand, const float* lpf, float* out,
                                void* workspace, int64_t workspace_bytes, int32_t b, int32_t f, int32_t c, int32_t h, int32_t w,
                                float sqrt_alpha, float sqrt_one_minus_alpha, i2v_stream_t stream) {
  I2V_CHECK_ARG(latents && init_noise && z_rand && lpf && out && workspace, "i2v_freeinit_mix: null pointer");
  I2V_CHECK_ARG(fi_sizes_ok(b, f, c, h, w),
                "i2v_freeinit_mix: not implemented for this problem (b %d f %d c %d h %d w %d: f in 1..%d, h and w in 1..%d, at most 2^30 "
                "values)", b, f, c, h, w, FI_MAX_F, FI_MAX_HW);
  const int64_t elems = (int64_t)b * f * c * h * w, bytes = elems * (int64_t)sizeof(float), need = elems * (int64_t)sizeof(float2);
  I2V_CHECK_ARG(workspace_bytes >= need, "i2v_freeinit_mix: workspace of %lld bytes, %lld needed (i2v_freeinit_workspace_bytes)",
                (long long)workspace_bytes, (long long)need);
  I2V_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "i2v_freeinit_mix: the workspace must be 8-byte aligned");
  I2V_CHECK_ARG(!fi_overlap(out, bytes, latents, bytes) && !fi_overlap(out, bytes, init_noise, bytes) &&
                    !fi_overlap(out, bytes, z_rand, bytes) && !fi_overlap(out, bytes, lpf, (int64_t)f * h * w * (int64_t)sizeof(float)),
                "i2v_freeinit_mix: out is a new tensor (it must not alias an input)");
  I2V_CHECK_ARG(!fi_overlap(workspace, need, out, bytes) && !fi_overlap(workspace, need, latents, bytes) &&
                    !fi_overlap(workspace, need, init_noise, bytes) && !fi_overlap(workspace, need, z_rand, bytes) &&
                    !fi_overlap(workspace, need, lpf, (int64_t)f * h * w * (int64_t)sizeof(float)),
                "i2v_freeinit_mix: the workspace must not overlap an operand");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  fi_args a{};
  a.lat = latents, a.noise = init_noise, a.zr = z_rand, a.lpf = lpf, a.out = out, a.ws = reinterpret_cast<float2*>(workspace);
  a.hh = h, a.ww = w, a.sa = sqrt_alpha, a.sb = sqrt_one_minus_alpha;
  a.scale = (float)(1.0 / ((double)f * (double)h * (double)w));
  const int64_t planes = (int64_t)b * f * c;
  // rows: [planes * h][w];  columns: [planes][h][w];  frames: [b][f][c * h * w]
  a.n = w, a.inner = 1, a.nlines = planes * h;
  fi_launch<FI_ROWS_FWD>(a, st);
  a.n = h, a.inner = w, a.nlines = planes * w;
  fi_launch<FI_AXIS_FWD>(a, st);
  a.n = f, a.inner = (int64_t)c * h * w, a.nlines = (int64_t)b * c * h * w;
  fi_launch<FI_FRAMES>(a, st);
  a.n = h, a.inner = w, a.nlines = planes * w;
  fi_launch<FI_AXIS_INV>(a, st);
  a.n = w, a.inner = 1, a.nlines = planes * h;
  fi_launch<FI_ROWS_INV>(a, st);
  return i2v_check_launch("i2v_freeinit_mix");
}
