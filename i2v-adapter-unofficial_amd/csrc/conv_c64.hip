// 3x3 / pad 1 / stride 1 convolution with Cin = Cout = 64 and a fused epilogue: the layer AutoencoderTiny (TAESD) and the Real-ESRGAN
// compact upscaler (SRVGGNetCompact) are made of (i2v_conv3x3_c64_f16 / i2v_conv3x3_c64_prelu_f16), and their entry mover
// (i2v_taesd_prep_f16).
//
//   out = act_out( act_mid(conv(x) + bias) + residual )            token-major fp16 [N, H, W, 64], fp32 arithmetic, one rounding
//
// act_mid is ReLU / identity (conv_c64_kernel<false>) or a per-channel PReLU v >= 0 ? v : slope[c] v (conv_c64_kernel<true>: the same
// kernel with 16 more registers, the lane's slopes held like its bias; ReLU and leaky ReLU are slope 0 and 0.1).
//
// conv_thin.hip's scheme at 64 output channels.  A workgroup of four waves owns an 8 x 16 pixel tile of one image; the tile WITH its
// halo (10 x 18 pixels x 128 B = 23 KB) is staged in LDS once and the nine taps are 16x16x32 MFMAs against SHIFTED reads of it:
//   D[16 output channels x 16 pixels of a tile row] += W_tap[16 x 32] X^T[32 x 16 pixels, shifted by the tap].
// Wave w owns tile rows 2 w, 2 w + 1 and all 64 output channels: 8 accumulators, 144 MFMAs per tile.
// The whole weight (64 x 576 fp16 = 72 KB) sits in LDS for the life of the workgroup, so the kernel is PERSISTENT over tiles (a
// workgroup per tile would move three times more weight than image): workgroup b walks tiles b, b + grid, ...; the next tile's halo
// is fetched into registers before the current tile's MFMAs and written to the other LDS buffer after them: one barrier per tile.
//
// LDS image: 120 KB = weights 72 KB + 2 halo tiles of 24 KB; one workgroup per CU.
//  * weights, in MFMA-fragment order: [tap 9][k-step 2][channel block 4][lane 64][8 fp16] -- the A fragment of a wave is ONE linear
//    1 KB ds_read_b128 (lane l at base + 16 l): conflict-free by construction.  The host packs that order once
//    (kernels.pack_conv_c64); the kernel copies it.  Row r = 4 q + e of channel block b is output channel 32 (b >> 1) + 8 q + 4 (b & 1) + e,
//    so that a lane's accumulators of blocks 2 h, 2 h + 1 are EIGHT CONSECUTIVE channels 32 h + 8 g ..: 16-byte stores.
//  * a halo tile, as 8 planes of 8 channels: [plane 8][slot 192][16 B], halo pixel hp = 18 hy + hx of plane c at slot hp ^ 2 (c >> 1).
//    The B fragment of lane (g = l >> 4, l15 = l & 15) in k-step s is plane 4 s + g of pixel hp0 + l15.  ds_read_b128 is served in
//    16-lane groups that MIX two values of g ({0-3, 12-15} of one with {4-11} of the next), and a plane is a multiple of 256 B, so the
//    16 lanes of a group read 16 consecutive pixels (mod the XOR, the same for planes 2 m and 2 m + 1): 16 distinct 16-byte slots of
//    the 256-byte bank row.  A pixel-major image (conv_thin's 144-byte pixels) cannot do that for the mixed groups: whatever the
//    pixel stride, lanes of plane g + 1 land on slots of plane g.  The XOR spreads the STORES: the 8 lanes that stage one pixel
//    (8 planes, the same slot without it) fall on 4 slots of the 128-byte store row -- 2-way, which a 16-byte store's own 13 cycles hide.
#include "common.h"

namespace {

constexpr int C6_C = 64;
constexpr int C6_TH = 8, C6_TW = 16;                     // output tile (rows x columns of pixels)
constexpr int C6_HH = C6_TH + 2, C6_HW = C6_TW + 2;      // with the halo
constexpr int C6_HP = C6_HH * C6_HW;                     // 180 halo pixels
constexpr int C6_PLANE = 192 * 16;                       // bytes of an 8-channel plane: 180 slots + the XOR's reach (<= 6), 12 x 256
constexpr int C6_TILE = 8 * C6_PLANE;                    // 24576
constexpr int C6_WPIECES = 9 * 2 * 4 * 64;               // 16-byte pieces of the packed weight: 4608
constexpr int C6_WBYTES = C6_WPIECES * 16;               // 73728
constexpr int C6_LDS = C6_WBYTES + 2 * C6_TILE;          // 122880
constexpr int C6_PIECES = C6_HP * 8;                     // 16-byte pieces of a halo tile: 1440
constexpr int C6_NLD = (C6_PIECES + 255) / 256;          // per thread: 6
static_assert((C6_HP - 1 | 6) < 192 && C6_PLANE % 256 == 0 && C6_LDS <= 160 * 1024, "LDS image");

// UP2 (conv_c64_kernel<true, true>, i2v_conv3x3_c64_up2_prelu_f16): x is the image at HALF the size and the convolution runs on its
// nearest-2x upsampling, which is never written: halo pixel (y, x) of the 2H x 2W grid is source pixel (y >> 1, x >> 1), zero outside
// the grid.  Only the fetch differs.
template <bool PRELU, bool UP2 = false>
__global__ __launch_bounds__(256, 1) void conv_c64_kernel(const i2v_conv_c64_params p, const int tiles_x, const int tiles_y, const int ntiles,
                                                          const float* __restrict__ slope) {
  extern __shared__ __attribute__((aligned(16))) char smem[];     // W fragments, then [2] halo tiles
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, l15 = lane & 15;
  char* const halo = smem + C6_WBYTES;
  const f16* __restrict__ X = reinterpret_cast<const f16*>(p.x);
  const int H = p.height, Wd = p.width;
  const int ldx = (int)p.ldx;
  const int64_t img_stride = UP2 ? (int64_t)(H >> 1) * (Wd >> 1) * p.ldx : (int64_t)H * Wd * p.ldx;

  // ---- weights into LDS: a straight copy of the packed image
  {
    const f16* __restrict__ W = reinterpret_cast<const f16*>(p.w);
    for (int i = tid; i < C6_WPIECES; i += 256) *reinterpret_cast<f16x8*>(smem + i * 16) = ld_global_16B(W + i * 8);
  }

  // ---- halo-tile staging: piece i of a thread = 16 bytes (8 channels) of one halo pixel; zero outside the image
  int hyx[C6_NLD], dst_off[C6_NLD];     // (hy << 8 | hx) and part * 8 are the piece's, whatever the tile; dst_off < 0: no piece
#pragma unroll
  for (int i = 0; i < C6_NLD; ++i) {
    const int piece = tid + 256 * i;
    const int hp = piece >> 3, part = piece & 7;
    const int hy = hp / C6_HW, hx = hp - hy * C6_HW;
    hyx[i] = hy << 8 | hx;
    dst_off[i] = piece < C6_PIECES ? part * C6_PLANE + ((hp ^ (2 * (part >> 1))) << 4) : -1;
  }
  const int part8 = (tid & 7) * 8;
  f16x8 st[C6_NLD];
  auto fetch = [&](int t) {
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, img = t / tiles_y;
    const f16* __restrict__ Xi = X + (int64_t)img * img_stride + part8;
#pragma unroll
    for (int i = 0; i < C6_NLD; ++i) {
      const int y = ty * C6_TH + (hyx[i] >> 8) - 1, x = tx * C6_TW + (hyx[i] & 255) - 1;
      const bool in = dst_off[i] >= 0 && y >= 0 && y < H && x >= 0 && x < Wd;
      if constexpr (UP2)
        st[i] = in ? ld_global_16B(Xi + ((y >> 1) * (Wd >> 1) + (x >> 1)) * ldx) : zero8();
      else
        st[i] = in ? ld_global_16B(Xi + (y * Wd + x) * ldx) : zero8();
    }
  };
  auto commit = [&](const int buf) {
#pragma unroll
    for (int i = 0; i < C6_NLD; ++i)
      if (dst_off[i] >= 0) *reinterpret_cast<f16x8*>(halo + buf * C6_TILE + dst_off[i]) = st[i];
  };

  // bias of this lane's channels 32 h + 8 g .. + 7
  float bv[2][8];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const f16x8 b = p.bias ? ld_global_16B(reinterpret_cast<const f16*>(p.bias) + 32 * h + 8 * g) : zero8();
#pragma unroll
    for (int j = 0; j < 8; ++j) bv[h][j] = (float)b[j];
  }
  // ... and, for the PReLU epilogue, their slopes (fp32 [64]: two 16-byte loads per half)
  float sv[2][8];
  if constexpr (PRELU) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x4 s0 = *reinterpret_cast<const f32x4*>(slope + 32 * h + 8 * g), s1 = *reinterpret_cast<const f32x4*>(slope + 32 * h + 8 * g + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) sv[h][j] = s0[j], sv[h][4 + j] = s1[j];
    }
  }
  const bool relu_mid = p.relu_mid != 0, relu_out = p.relu_out != 0;
  const f16* __restrict__ R = reinterpret_cast<const f16*>(p.residual);
  f16* __restrict__ O = reinterpret_cast<f16*>(p.out);

  int t = blockIdx.x;
  fetch(t);
  commit(0);
  __syncthreads();

  for (int it = 0; t < ntiles; t += gridDim.x, ++it) {
    const int tn = t + gridDim.x;
    if (tn < ntiles) fetch(tn);
    const char* hb = halo + (it & 1) * C6_TILE;
    // this lane's two output pixels (rows 2 wave + r, column l15 of the tile) and their residual, fetched ahead of the MFMAs
    int64_t pix[2];
    bool live[2];
    f16x8 rr[2][2];
    {
      int q = t;
      const int tx = q % tiles_x;
      q /= tiles_x;
      const int ty = q % tiles_y, img = q / tiles_y;
      const int x = tx * C6_TW + l15;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int y = ty * C6_TH + 2 * wave + r;
        live[r] = y < H && x < Wd;
        pix[r] = ((int64_t)img * H + y) * Wd + x;
#pragma unroll
        for (int h = 0; h < 2; ++h) rr[r][h] = (R != nullptr && live[r]) ? ld_global_16B(R + pix[r] * p.ldr + 32 * h + 8 * g) : zero8();
      }
    }
    f32x4 acc[4][2];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b][0] = acc[b][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    // step k = 2 tap + s of the contraction.  The fragments of step k + 1 are read while the MFMAs of step k run: with one wave per
    // SIMD nothing else hides an LDS read, and left to itself the compiler reads each fragment just ahead of its MFMA.
    //   A: W[row l15 of channel block b][k-step] -- linear in the lane.   B: X[pixel (row 2 wave + r + dy, column l15 + dx)][plane 4 s + g]
    f16x8 wf[2][4], xf[2][2];
    auto read_step = [&](const int k, f16x8 (&w)[4], f16x8 (&x)[2]) {
      const int tap = k >> 1, s = k & 1, dy = tap / 3, dx = tap - 3 * dy;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int hp = (2 * wave + r + dy) * C6_HW + l15 + dx;
        x[r] = *reinterpret_cast<const f16x8*>(hb + (4 * s + g) * C6_PLANE + ((hp ^ (4 * s + 2 * (g >> 1))) << 4));
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) w[b] = *reinterpret_cast<const f16x8*>(smem + ((k * 4 + b) * 64 + lane) * 16);
    };
    read_step(0, wf[0], xf[0]);
#pragma unroll
    for (int k = 0; k < 18; ++k) {
      if (k + 1 < 18) read_step(k + 1, wf[(k + 1) & 1], xf[(k + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        acc[b][0] = mfma16x16x32(wf[k & 1][b], xf[k & 1][0], acc[b][0]);
        acc[b][1] = mfma16x16x32(wf[k & 1][b], xf[k & 1][1], acc[b][1]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }

    // ---- D[channel 32 h + 8 g + 4 (b & 1) + e][pixel l15] -> act_out(act_mid(. + bias) + residual), 16 bytes per lane and store
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (live[r]) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          f16x8 o;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float v = acc[2 * h + (j >> 2)][r][j & 3] + bv[h][j];
            if constexpr (PRELU)
              v = v >= 0.f ? v : sv[h][j] * v;
            else if (relu_mid)
              v = fmaxf(v, 0.f);
            v += (float)rr[r][h][j];              // (zeros without a residual: v + 0 is v, and -0 + 0 = +0 is the same fp16 number)
            o[j] = (f16)(relu_out ? fmaxf(v, 0.f) : v);
          }
          *reinterpret_cast<f16x8*>(O + pix[r] * p.ldo + 32 * h + 8 * g) = o;
        }
      }
    }

    if (tn < ntiles) commit((it + 1) & 1);      // the other buffer was last read in iteration it - 1, closed by its barrier
    lds_barrier();                              // (LDS only: the tile's stores stay in flight across it, common.h)
  }
}

// NCHW fp32 / fp16 -> token-major fp16 [N, H, W, 64] (pixel stride ld_dst), channels >= c zero, through one of four maps
template <bool F32>
__global__ __launch_bounds__(256) void taesd_prep_kernel(const void* __restrict__ src_, f16* __restrict__ dst, const int64_t ld_dst,
                                                         const int64_t items, const int c, const int hw, const int mode) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += stride) {
    const int part = (int)(i & 7);
    const int64_t pix = i >> 3;                 // image * hw + pixel
    const int64_t img = pix / hw;
    const int64_t s0 = (img * c + part * 8) * hw + (pix - img * hw);
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = 0.f;
      if (part * 8 + j < c) {
        v = F32 ? reinterpret_cast<const float*>(src_)[s0 + (int64_t)j * hw] : (float)reinterpret_cast<const f16*>(src_)[s0 + (int64_t)j * hw];
        if (mode == I2V_TAESD_PREP_UNIT)
          v = (v + 1.0f) * 0.5f;
        else if (mode == I2V_TAESD_PREP_UNIT_CLAMP)
          v = fminf(fmaxf((v + 1.0f) * 0.5f, 0.0f), 1.0f);
        else if (mode == I2V_TAESD_PREP_CLAMP)
          v = 3.0f * tanhf(v / 3.0f);
      }
      o[j] = (f16)v;
    }
    *reinterpret_cast<f16x8*>(dst + pix * ld_dst + part * 8) = o;
  }
}

}  // namespace

namespace {

// the argument checks and the launch of the entry points: `fn` names the entry in the messages, `prelu` / `up2` select the instantiation
// (up2: height and width are the OUTPUT's, both even; x holds n_img images of half that size)
int conv_c64_launch(const char* fn, const i2v_conv_c64_params* p, const bool prelu, const void* slope, i2v_stream_t stream,
                    const bool up2 = false) {
  I2V_CHECK_ARG(p != nullptr, "%s: null params", fn);
  I2V_CHECK_ARG(p->x && p->w && p->out, "%s: null pointer", fn);
  I2V_CHECK_ARG(p->cin == C6_C && p->cout == C6_C, "%s: Cin %d, Cout %d: this kernel is the 64 -> 64 convolution", fn, p->cin,
                p->cout);
  I2V_CHECK_ARG(p->n_img >= 1 && p->height >= 1 && p->width >= 1, "%s: n %d, h %d, w %d", fn, p->n_img, p->height, p->width);
  const int64_t lim = (int64_t)1 << 31;
  I2V_CHECK_ARG(p->ldx >= C6_C && p->ldx % 8 == 0 && p->ldo >= C6_C && p->ldo % 8 == 0 && p->ldx < (1 << 20) && p->ldo < (1 << 20),
                "%s: pixel strides ldx %lld, ldo %lld must be >= 64 and multiples of 8", fn, (long long)p->ldx, (long long)p->ldo);
  I2V_CHECK_ARG(p->residual == nullptr || (p->ldr >= C6_C && p->ldr % 8 == 0 && p->ldr < (1 << 20)),
                "%s: residual pixel stride %lld must be >= 64 and a multiple of 8", fn, (long long)p->ldr);
  I2V_CHECK_ARG(i2v_al16(p->x) && i2v_al16(p->w) && i2v_al16(p->out) && i2v_al16(p->bias) && i2v_al16(p->residual),
                "%s: operands must be 16-byte aligned", fn);
  I2V_CHECK_ARG(!up2 || (p->height % 2 == 0 && p->width % 2 == 0), "%s: output height %d and width %d must be even (twice the source's)", fn,
                p->height, p->width);
  const int64_t hw = (int64_t)p->height * p->width, pixels = hw * p->n_img;
  I2V_CHECK_ARG(hw * p->ldx < lim && pixels < lim, "%s: problem too large", fn);
  const int64_t xb = (((up2 ? pixels / 4 : pixels) - 1) * p->ldx + C6_C) * 2, ob = ((pixels - 1) * p->ldo + C6_C) * 2;      // bytes from the first to the last element
  // other workgroups read x as halo while this one stores: out may not be x
  I2V_CHECK_ARG(!i2v_overlap(p->out, ob, p->x, xb), "%s: out overlaps x (other workgroups read x as halo)", fn);
  I2V_CHECK_ARG(!i2v_overlap(p->out, ob, p->w, C6_WBYTES) && (p->bias == nullptr || !i2v_overlap(p->out, ob, p->bias, C6_C * 2)),
                "%s: out overlaps the weights", fn);
  // every element of the residual is read by the lane that then stores it: out may BE the residual, and nothing in between
  I2V_CHECK_ARG(p->residual == nullptr || (p->residual == p->out && p->ldr == p->ldo) || !i2v_overlap(p->out, ob, p->residual, ((pixels - 1) * p->ldr + C6_C) * 2),
                "%s: out overlaps the residual without being it", fn);
  I2V_CHECK_ARG(p->max_workgroups >= 0, "%s: max_workgroups %d", fn, p->max_workgroups);
  if (prelu) {
    I2V_CHECK_ARG(slope != nullptr && i2v_al16(slope), "%s: slope must be 64 fp32 values, non-null and 16-byte aligned", fn);
    I2V_CHECK_ARG(p->relu_mid == 0, "%s: relu_mid must be 0 (act_mid is the PReLU)", fn);
    I2V_CHECK_ARG(!i2v_overlap(p->out, ob, slope, C6_C * 4), "%s: out overlaps slope", fn);
  }
  const int tiles_x = (int)i2v_cdiv(p->width, C6_TW), tiles_y = (int)i2v_cdiv(p->height, C6_TH);
  const int64_t ntiles = (int64_t)p->n_img * tiles_x * tiles_y;
  I2V_CHECK_ARG(ntiles < lim - (1 << 20), "%s: problem too large", fn);
  const void* kernel = up2     ? reinterpret_cast<const void*>(conv_c64_kernel<true, true>)
                       : prelu ? reinterpret_cast<const void*>(conv_c64_kernel<true>)
                               : reinterpret_cast<const void*>(conv_c64_kernel<false>);
  const int cus = i2v_big_lds_kernel_cus(kernel, C6_LDS);
  if (cus <= 0) I2V_FAIL(I2V_ERR_UNSUPPORTED, "%s: the device refuses %d bytes of LDS", fn, C6_LDS);
  int64_t grid = p->max_workgroups > 0 ? p->max_workgroups : cus;
  if (grid > ntiles) grid = ntiles;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (up2)
    hipLaunchKernelGGL((conv_c64_kernel<true, true>), dim3((unsigned)grid), dim3(256), C6_LDS, st, *p, tiles_x, tiles_y, (int)ntiles,
                       reinterpret_cast<const float*>(slope));
  else if (prelu)
    hipLaunchKernelGGL(conv_c64_kernel<true>, dim3((unsigned)grid), dim3(256), C6_LDS, st, *p, tiles_x, tiles_y, (int)ntiles,
                       reinterpret_cast<const float*>(slope));
  else
    hipLaunchKernelGGL(conv_c64_kernel<false>, dim3((unsigned)grid), dim3(256), C6_LDS, st, *p, tiles_x, tiles_y, (int)ntiles,
                       static_cast<const float*>(nullptr));
  return i2v_check_launch(fn);
}

}  // namespace

extern "C" int i2v_conv3x3_c64_f16(const i2v_conv_c64_params* p, i2v_stream_t stream) {
  return conv_c64_launch("i2v_conv3x3_c64_f16", p, false, nullptr, stream);
}

extern "C" int i2v_conv3x3_c64_prelu_f16(const i2v_conv_c64_params* p, const void* slope, i2v_stream_t stream) {
  return conv_c64_launch("i2v_conv3x3_c64_prelu_f16", p, true, slope, stream);
}

extern "C" int i2v_conv3x3_c64_up2_prelu_f16(const i2v_conv_c64_params* p, const void* slope, i2v_stream_t stream) {
  return conv_c64_launch("i2v_conv3x3_c64_up2_prelu_f16", p, true, slope, stream, true);
}

extern "C" int i2v_taesd_prep_f16(const void* src, int32_t src_is_f32, void* dst, int64_t ld_dst, int32_t n, int32_t c, int32_t hw, int32_t mode,
                                  i2v_stream_t stream) {
  I2V_CHECK_ARG(src && dst, "i2v_taesd_prep_f16: null pointer");
  I2V_CHECK_ARG(n >= 1 && hw >= 1 && c >= 1 && c <= C6_C, "i2v_taesd_prep_f16: n %d, c %d (1..64), hw %d", n, c, hw);
  I2V_CHECK_ARG(mode == I2V_TAESD_PREP_IDENTITY || mode == I2V_TAESD_PREP_UNIT || mode == I2V_TAESD_PREP_CLAMP || mode == I2V_TAESD_PREP_UNIT_CLAMP,
                "i2v_taesd_prep_f16: mode %d", mode);
  I2V_CHECK_ARG(ld_dst >= C6_C && ld_dst % 8 == 0 && ld_dst < (1 << 20) && i2v_al16(dst),
                "i2v_taesd_prep_f16: dst must be 16-byte aligned with a pixel stride >= 64 that is a multiple of 8");
  const int64_t pixels = (int64_t)n * hw;
  I2V_CHECK_ARG(pixels < ((int64_t)1 << 31), "i2v_taesd_prep_f16: problem too large");
  I2V_CHECK_ARG(!i2v_overlap(dst, ((pixels - 1) * ld_dst + C6_C) * 2, src, pixels * c * (src_is_f32 ? 4 : 2)), "i2v_taesd_prep_f16: dst overlaps src");
  const int64_t items = pixels * 8;
  const unsigned grid = i2v_ew_grid(items, 256, 4096);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (src_is_f32)
    hipLaunchKernelGGL(taesd_prep_kernel<true>, dim3(grid), dim3(256), 0, st, src, reinterpret_cast<f16*>(dst), ld_dst, items, c, hw, mode);
  else
    hipLaunchKernelGGL(taesd_prep_kernel<false>, dim3(grid), dim3(256), 0, st, src, reinterpret_cast<f16*>(dst), ld_dst, items, c, hw, mode);
  return i2v_check_launch("i2v_taesd_prep_f16");
}
