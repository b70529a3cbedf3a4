// Blend-and-stitch of the tiled VAE (diffusers 0.24 AutoencoderKL.tiled_decode / tiled_encode, behind the reference's
// enable_vae_tiling, pipe:139-153): one launch per tile writes that tile's crop rectangle of the stitched fp32 NCHW image.
//
// diffusers blends the tile grid in raster order and IN PLACE -- tile = blend_v(tile above, tile, E), then blend_h(tile to the left,
// tile, E), then tile[:limit, :limit] is kept -- so the neighbour a tile reads has itself been blended.  With an overlap factor
// <= 1/3 a tile that has a successor is at least 2 E long, the rows / columns it hands on (its last e <= E) lie outside its own blend
// zone along the same axis, and every output element is a function of at most four RAW tiles: T (own), U (above), L (left), UL
// (diagonal).  With ev = min(U.h, T.h, E), eh = min(L.w, T.w, E), uy = U.h - ev + y, lx = L.w - eh + x, lerp(a, b, w) = a (1 - w) + b w:
//
//   FU  = x < eh ? lerp(UL[uy, lx], U[uy, x], x / eh) : U[uy, x]          (U after its own horizontal blend)
//   v   = y < ev ? lerp(FU, T[y, x], y / ev)          : T[y, x]
//   FL  = y < ev ? lerp(UL[uy, lx], L[y, lx], y / ev) : L[y, lx]          (L after its own vertical blend)
//   out = x < eh ? lerp(FL, v, x / eh)                : v
//
// No input is modified, launches of one grid are independent of each other, and outside the blend zones the source passes through
// bit for bit (converted to fp32).  The launch also is the layout edge: sources are token-major [n, h, w, ld] (fp32: the decoder's
// conv_out; fp16: quant_conv's GEMM output), the destination is NCHW -- tokens_to_nchw, both blends, the crop and both concatenations
// in one pass.
//
// Pure HBM traffic: a thread owns one output pixel and up to 8 (fp16) / 4 (fp32) consecutive channels of it.  The source pixel is one
// vector load along ld (16 B; 12 B for the decoder's 3-channel fp32 image, whose pixels are 12 B apart), consecutive lanes take
// consecutive x, so a wave reads one contiguous span of the source row and stores one 256-byte run per channel plane.
#include "common.h"

namespace {

constexpr int VT_BX = 64;      // pixels along x per workgroup (one wave = one row segment)
constexpr int VT_BY = 4;       // rows per workgroup
constexpr int VT_SCALAR = 0, VT_VECTOR = 1, VT_F32X3 = 3;

struct __attribute__((packed, aligned(4))) vt_f32x3 {
  float a, b, c;
};

template <bool F32>
struct vt_width {
  static constexpr int value = F32 ? 4 : 8;
};

// channels cb .. cb + W - 1 of pixel `px` of a token-major image, as fp32 (channels >= c read as 0 in the scalar form)
template <bool F32, int VEC>
__device__ __forceinline__ void vt_load(const void* __restrict__ base, int64_t px, int ld, int cb, int c, float (&v)[vt_width<F32>::value]) {
  constexpr int W = vt_width<F32>::value;
  const int64_t off = px * ld + cb;
  if constexpr (VEC == VT_F32X3) {
    const vt_f32x3 t = *reinterpret_cast<const vt_f32x3*>(reinterpret_cast<const float*>(base) + off);
    v[0] = t.a, v[1] = t.b, v[2] = t.c, v[3] = 0.f;
  } else if constexpr (VEC == VT_VECTOR && F32) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + off);
#pragma unroll
    for (int j = 0; j < W; ++j) v[j] = t[j];
  } else if constexpr (VEC == VT_VECTOR) {
    const f16x8 t = *reinterpret_cast<const f16x8*>(reinterpret_cast<const f16*>(base) + off);
#pragma unroll
    for (int j = 0; j < W; ++j) v[j] = (float)t[j];
  } else {
#pragma unroll
    for (int j = 0; j < W; ++j) {
      v[j] = 0.f;
      if (cb + j < c) v[j] = F32 ? reinterpret_cast<const float*>(base)[off + j] : (float)reinterpret_cast<const f16*>(base)[off + j];
    }
  }
}

template <int W>
__device__ __forceinline__ void vt_lerp(const float (&a)[W], float (&b)[W], float w) {      // b = a (1 - w) + b w
  const float wa = 1.0f - w;
#pragma unroll
  for (int j = 0; j < W; ++j) b[j] = a[j] * wa + b[j] * w;
}

template <bool F32, int VEC>
__global__ __launch_bounds__(VT_BX* VT_BY) void vae_tile_blend_kernel(const void* __restrict__ tile, const void* __restrict__ up,
                                                                      const void* __restrict__ left, const void* __restrict__ upleft,
                                                                      int th, int tw, int ld, int c, int up_h, int left_w, int ev, int eh,
                                                                      int crop_h, int crop_w, float* __restrict__ out, int out_h,
                                                                      int out_w, int oy, int ox, int chunks) {
  constexpr int W = vt_width<F32>::value;
  const int x = (int)blockIdx.x * VT_BX + (int)(threadIdx.x & (VT_BX - 1));
  const int y = (int)blockIdx.y * VT_BY + (int)(threadIdx.x / VT_BX);
  if (x >= crop_w || y >= crop_h) return;
  const int img = (int)blockIdx.z / chunks, cb = ((int)blockIdx.z - img * chunks) * W;

  float v[W];
  vt_load<F32, VEC>(tile, ((int64_t)img * th + y) * tw + x, ld, cb, c, v);
  const bool inv = y < ev, inh = x < eh;                       // ev / eh are 0 without the neighbour
  if (inv || inh) {
    const int uy = up_h - ev + y, lx = left_w - eh + x;
    const float wy = inv ? (float)y / (float)ev : 1.0f, wx = inh ? (float)x / (float)eh : 1.0f;
    const bool corner = inv && inh && upleft != nullptr;
    float d[W];
    if (corner) vt_load<F32, VEC>(upleft, ((int64_t)img * up_h + uy) * left_w + lx, ld, cb, c, d);
    if (inv) {
      float u[W];
      vt_load<F32, VEC>(up, ((int64_t)img * up_h + uy) * tw + x, ld, cb, c, u);
      if (corner) vt_lerp<W>(d, u, wx);
      vt_lerp<W>(u, v, wy);
    }
    if (inh) {
      float l[W];
      vt_load<F32, VEC>(left, ((int64_t)img * th + y) * left_w + lx, ld, cb, c, l);
      if (corner) vt_lerp<W>(d, l, wy);
      vt_lerp<W>(l, v, wx);
    }
  }
  float* dst = out + (((int64_t)img * c + cb) * out_h + (oy + y)) * out_w + (ox + x);
  const int64_t plane = (int64_t)out_h * out_w;
#pragma unroll
  for (int j = 0; j < W; ++j)
    if (cb + j < c) dst[j * plane] = v[j];
}

template <bool F32, int VEC>
void vt_launch(dim3 grid, hipStream_t st, const void* tile, const void* up, const void* left, const void* upleft, int th, int tw, int ld,
               int c, int up_h, int left_w, int ev, int eh, int crop_h, int crop_w, float* out, int out_h, int out_w, int oy, int ox,
               int chunks) {
  hipLaunchKernelGGL((vae_tile_blend_kernel<F32, VEC>), grid, dim3(VT_BX * VT_BY), 0, st, tile, up, left, upleft, th, tw, ld, c, up_h,
                     left_w, ev, eh, crop_h, crop_w, out, out_h, out_w, oy, ox, chunks);
}

}  // namespace

extern "C" int i2v_vae_tile_blend(const void* tile, const void* up, const void* left, const void* upleft, int32_t src_is_f32, int32_t n,
                                  int32_t th, int32_t tw, int64_t ld, int32_t c, int32_t up_h, int32_t left_w, int32_t blend_extent,
                                  int32_t limit, void* out, int32_t out_h, int32_t out_w, int32_t oy, int32_t ox, i2v_stream_t stream) {
  I2V_CHECK_ARG(tile && out, "i2v_vae_tile_blend: null pointer");
  I2V_CHECK_ARG(n > 0 && th > 0 && tw > 0 && c > 0 && out_h > 0 && out_w > 0, "i2v_vae_tile_blend: n %d th %d tw %d c %d out %d x %d", n, th,
                tw, c, out_h, out_w);
  I2V_CHECK_ARG(ld >= c && ld < ((int64_t)1 << 20), "i2v_vae_tile_blend: c %d > ld %lld (or ld too large)", c, (long long)ld);
  I2V_CHECK_ARG(limit > 0, "i2v_vae_tile_blend: limit %d must be positive", limit);
  I2V_CHECK_ARG(blend_extent > 0, "i2v_vae_tile_blend: blend_extent %d must be positive", blend_extent);
  I2V_CHECK_ARG(upleft == nullptr || (up != nullptr && left != nullptr), "i2v_vae_tile_blend: upleft comes with both up and left");
  I2V_CHECK_ARG(up == nullptr || up_h > 0, "i2v_vae_tile_blend: up_h %d of the tile above", up_h);
  I2V_CHECK_ARG(left == nullptr || left_w > 0, "i2v_vae_tile_blend: left_w %d of the tile to the left", left_w);
  const int crop_h = th < limit ? th : limit, crop_w = tw < limit ? tw : limit;
  I2V_CHECK_ARG(oy >= 0 && ox >= 0 && (int64_t)oy + crop_h <= out_h && (int64_t)ox + crop_w <= out_w,
                "i2v_vae_tile_blend: the crop %d x %d at (%d, %d) leaves the %d x %d destination", crop_h, crop_w, oy, ox, out_h, out_w);
  const int64_t lim = (int64_t)1 << 40;
  I2V_CHECK_ARG((int64_t)n * c * out_h * out_w < lim && (int64_t)n * th * tw * ld < lim &&
                    (up == nullptr || (int64_t)n * up_h * tw * ld < lim) && (left == nullptr || (int64_t)n * th * left_w * ld < lim) &&
                    (upleft == nullptr || (int64_t)n * up_h * left_w * ld < lim),
                "i2v_vae_tile_blend: problem too large");
  const int e_up = up ? (up_h < th ? up_h : th) : 0, e_left = left ? (left_w < tw ? left_w : tw) : 0;
  const int ev = e_up < blend_extent ? e_up : blend_extent, eh = e_left < blend_extent ? e_left : blend_extent;

  const bool f32 = src_is_f32 != 0;
  const int w = f32 ? 4 : 8;
  int vec = VT_SCALAR;
  if (f32 && ld == 3 && c == 3)
    vec = VT_F32X3;
  else if (ld % w == 0 && i2v_al16(tile) && i2v_al16(up) && i2v_al16(left) && i2v_al16(upleft))
    vec = VT_VECTOR;
  const int chunks = vec == VT_F32X3 ? 1 : (int)i2v_cdiv(c, w);
  const int64_t gy = i2v_cdiv(crop_h, VT_BY), gz = (int64_t)n * chunks;
  I2V_CHECK_ARG(gy <= 65535 && gz <= 65535, "i2v_vae_tile_blend: %d rows / %d images x %d channel chunks exceed the grid", crop_h, n, chunks);
  const dim3 grid((unsigned)i2v_cdiv(crop_w, VT_BX), (unsigned)gy, (unsigned)gz);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* o = reinterpret_cast<float*>(out);
#define VT_GO(F32, VEC) \
  vt_launch<F32, VEC>(grid, st, tile, up, left, upleft, th, tw, (int)ld, c, up_h, left_w, ev, eh, crop_h, crop_w, o, out_h, out_w, oy, ox, chunks)
  if (vec == VT_F32X3)
    VT_GO(true, VT_F32X3);
  else if (f32 && vec == VT_VECTOR)
    VT_GO(true, VT_VECTOR);
  else if (f32)
    VT_GO(true, VT_SCALAR);
  else if (vec == VT_VECTOR)
    VT_GO(false, VT_VECTOR);
  else
    VT_GO(false, VT_SCALAR);
#undef VT_GO
  return i2v_check_launch("i2v_vae_tile_blend");
}
