// 3x3 / pad 1 / stride 1 convolution of the FIRST cin channels of a token-major fp16 buffer, cin in {64, 96, 128, 160, 192}, to 32 or
// 64 output channels, with a leaky ReLU and two scaled residual stages in the epilogue: the layer of an RRDBNet dense block
// (Real-ESRGAN x4plus, upscaler.RRDBNet; i2v_conv3x3_dense_f16).
//
//   v   = lrelu(conv3x3(x[..., 0:cin]) + bias; slope)
//   out = fp16( s2 * (s1 * v + r1) + r2 )                      fp32 arithmetic, one rounding
//
// A dense block lives in ONE buffer [N, H, W, 192]: channels 0..63 are its input, 64..191 are x1..x4, and torch.cat never runs.
// Convolutions 1..4 write 32 channels of the buffer they read, at channel offset cin (other workgroups read channels < cin of the same
// pixels as halo meanwhile: disjoint bytes); conv5 writes 64 channels of the next block's buffer with `0.2 x5 + x` (and, closing an
// RRDB, `0.2 (.) + x0`) in its epilogue.
//
// conv_c64.hip's scheme with a contraction that is walked in 32-channel CHUNKS.  A workgroup of four waves owns a 16 x 16 pixel
// tile of one image and 32 output channels; wave w owns tile rows 4 w .. 4 w + 3: 2 channel blocks x 4 rows = 8 accumulators.  A step
// of the contraction (one tap of one chunk) reads 2 weight fragments and 4 pixel fragments for 8 MFMAs: 0.75 ds_read_b128 per MFMA,
// the c64 kernel's rate (two rows per wave would be 4 reads per 4 MFMAs, the LDS array's limit).
// The 32 output channels' whole weight (9 cin 32 fp16: 36 .. 108 KB) sits in LDS for the life of the workgroup, so the kernel is
// PERSISTENT over tiles.  A 64-channel output is two halves: with two or more workgroups the even ones own half 0 and the odd ones
// half 1 (each copies its weight once); a single workgroup walks the tiles twice.
// The halo tile of ONE chunk (18 x 18 pixels x 64 B = 20.3 KB) is staged at a time, double-buffered: the next chunk (of this tile or
// the first of the next) is fetched into registers before the current chunk's 72 MFMAs and written to the other buffer after them:
// one barrier per chunk.  No channel >= cin is ever read.
//
// LDS image: 576 cin + 2 x 21504 bytes = 78 .. 150 KB; one workgroup per CU.
//  * weights, in MFMA-fragment order: [chunk cin / 32][tap 9][channel block 2][lane 64][8 fp16] -- the A fragment of a wave is ONE
//    linear 1 KB ds_read_b128.  The host packs that order once (kernels.pack_conv_dense), halves one after the other.  Row r = 4 q + e
//    of channel block b is output channel 8 q + 4 b + e of the half, so that a lane's accumulators of blocks 0, 1 are EIGHT
//    CONSECUTIVE channels 8 g ..: 16-byte stores.
//  * a halo chunk, as 4 planes of 8 channels: [plane 4][slot 336][16 B], halo pixel hp = 18 hy + hx of plane c at slot hp ^ 2 (c >> 1):
//    conv_c64.hip's layout (its first four planes), conflict-free for the same reason.
#include "common.h"

namespace {

constexpr int CD_TH = 16, CD_TW = 16;                    // output tile (rows x columns of pixels)
constexpr int CD_HH = CD_TH + 2, CD_HW = CD_TW + 2;      // with the halo
constexpr int CD_HP = CD_HH * CD_HW;                     // 324 halo pixels
constexpr int CD_PLANE = 336 * 16;                       // bytes of an 8-channel plane: 324 slots + the XOR's reach (<= 2), 21 x 256
constexpr int CD_CHUNK = 4 * CD_PLANE;                   // 21504: a 32-channel halo chunk
constexpr int CD_WSTEP = 2 * 64 * 16;                    // bytes of one (chunk, tap) of the packed weight: 2 channel blocks
constexpr int CD_MAXCIN = 192;
constexpr int CD_LDS_MAX = CD_MAXCIN / 32 * 9 * CD_WSTEP + 2 * CD_CHUNK;      // 153600
constexpr int CD_PIECES = CD_HP * 4;                     // 16-byte pieces of a halo chunk: 1296
constexpr int CD_NLD = (CD_PIECES + 255) / 256;          // per thread: 6
static_assert((CD_HP - 1 | 2) < 336 && CD_PLANE % 256 == 0 && CD_LDS_MAX <= 160 * 1024, "LDS image");

// WIDE: the closing convolution's form -- one or two halves of 32 output channels and the two residual stages; otherwise (a block's
// convolutions 1..4: 32 channels, s1 = s2 = 1, no residual) the epilogue is the leaky ReLU alone.
template <bool WIDE>
__global__ __launch_bounds__(256, 1) void conv_dense_kernel(const i2v_conv_dense_params p, const int tiles_x, const int tiles_y,
                                                            const int ntiles, const int groups) {
  extern __shared__ __attribute__((aligned(16))) char smem[];     // W fragments of one half, then [2] halo chunks
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, l15 = lane & 15;
  const int nchunk = p.cin >> 5, nhalves = WIDE ? p.cout >> 5 : 1;
  const int wbytes = nchunk * 9 * CD_WSTEP;
  char* const halo = smem + wbytes;
  const f16* __restrict__ X = reinterpret_cast<const f16*>(p.x);
  const int H = p.height, Wd = p.width;
  const int ldx = (int)p.ldx;
  const int64_t img_stride = (int64_t)H * Wd * p.ldx;
  const int gs = WIDE ? groups >> 1 : 0;      // groups is 1 or 2
  const int grp = blockIdx.x & gs, wg = blockIdx.x >> gs, nwg = gridDim.x >> gs;

  // ---- halo-chunk staging: piece i of a thread = 16 bytes (8 channels) of one halo pixel; zero outside the image
  int hyx[CD_NLD], dst_off[CD_NLD];     // (hy << 8 | hx) and part * 8 are the piece's, whatever the tile; dst_off < 0: no piece
#pragma unroll
  for (int i = 0; i < CD_NLD; ++i) {
    const int piece = tid + 256 * i;
    const int hp = piece >> 2, part = piece & 3;
    const int hy = hp / CD_HW, hx = hp - hy * CD_HW;
    hyx[i] = hy << 8 | hx;
    dst_off[i] = piece < CD_PIECES ? part * CD_PLANE + ((hp ^ (2 * (part >> 1))) << 4) : -1;
  }
  const int part8 = (tid & 3) * 8;
  f16x8 st[CD_NLD];
  auto fetch = [&](int t, const int c) {
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, img = t / tiles_y;
    const f16* __restrict__ Xi = X + (int64_t)img * img_stride + 32 * c + part8;
#pragma unroll
    for (int i = 0; i < CD_NLD; ++i) {
      const int y = ty * CD_TH + (hyx[i] >> 8) - 1, x = tx * CD_TW + (hyx[i] & 255) - 1;
      const bool in = dst_off[i] >= 0 && y >= 0 && y < H && x >= 0 && x < Wd;
      st[i] = in ? ld_global_16B(Xi + (y * Wd + x) * ldx) : zero8();
    }
  };
  auto commit = [&](const int buf) {
#pragma unroll
    for (int i = 0; i < CD_NLD; ++i)
      if (dst_off[i] >= 0) *reinterpret_cast<f16x8*>(halo + buf * CD_CHUNK + dst_off[i]) = st[i];
  };

  // pixel index of row 4 wave + r, column l15 of tile t, and whether it is inside the image
  auto locate = [&](int t, const int r, int64_t& pix) {
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, img = t / tiles_y;
    const int x = tx * CD_TW + l15, y = ty * CD_TH + 4 * wave + r;
    pix = ((int64_t)img * H + y) * Wd + x;
    return y < H && x < Wd;
  };
  const float slope = p.slope, s1 = p.s1, s2 = p.s2;
  const f16* __restrict__ R1 = reinterpret_cast<const f16*>(p.r1);
  const f16* __restrict__ R2 = reinterpret_cast<const f16*>(p.r2);
  f16* __restrict__ O = reinterpret_cast<f16*>(p.out);

  for (int half = grp; half < nhalves; half += 1 + gs) {
    const int ch0 = 32 * half + 8 * g;      // this lane's eight output channels
    __syncthreads();                        // (a second half: every wave is done with the first one's weights and halo)
    // ---- this half's weights into LDS: a straight copy of the packed image
    {
      const f16* __restrict__ W = reinterpret_cast<const f16*>(p.w) + (int64_t)half * (wbytes >> 1);
      for (int i = tid; i < (wbytes >> 4); i += 256) *reinterpret_cast<f16x8*>(smem + i * 16) = ld_global_16B(W + i * 8);
    }
    float bv[8];
    {
      const f16x8 b = p.bias ? ld_global_16B(reinterpret_cast<const f16*>(p.bias) + ch0) : zero8();
#pragma unroll
      for (int j = 0; j < 8; ++j) bv[j] = (float)b[j];
    }

    int t = wg;                             // (the host launches no workgroup without a tile)
    fetch(t, 0);
    commit(0);
    __syncthreads();

    for (int it = 0; t < ntiles; t += nwg) {
      // this lane's residuals of its four output pixels (rows 4 wave + r, column l15 of the tile), fetched ahead of the MFMAs.  A pixel
      // outside the image reads the nearest one inside instead (and stores nothing): a per-lane condition on the load would hold its
      // lane mask in scalar registers until the value arrives, eight of them across the MFMAs.
      f16x8 rr1[4], rr2[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) rr1[r] = rr2[r] = zero8();
      if constexpr (WIDE) {
        int q = t;
        const int tx = q % tiles_x;
        q /= tiles_x;
        const int ty = q % tiles_y, img = q / tiles_y;
        const int x = min(tx * CD_TW + l15, Wd - 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t pix = ((int64_t)img * H + min(ty * CD_TH + 4 * wave + r, H - 1)) * Wd + x;
          if (R1 != nullptr) rr1[r] = ld_global_16B(R1 + pix * p.ldr1 + ch0);
          if (R2 != nullptr) rr2[r] = ld_global_16B(R2 + pix * p.ldr2 + ch0);
        }
      }
      f32x4 acc[2][4];
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[b][r] = f32x4{0.f, 0.f, 0.f, 0.f};

      for (int c = 0; c < nchunk; ++c, ++it) {
        // the next chunk: of this tile, or the first of this workgroup's next tile
        const int tn = c + 1 < nchunk ? t : t + nwg, cn = c + 1 < nchunk ? c + 1 : 0;
        if (tn < ntiles) fetch(tn, cn);
        const char* hb = halo + (it & 1) * CD_CHUNK;
        const char* wb = smem + c * 9 * CD_WSTEP;
        // step = tap of this chunk.  The fragments of step k + 1 are read while the MFMAs of step k run (conv_c64.hip).
        //   A: W[row l15 of channel block b][chunk, tap] -- linear in the lane.   B: X[pixel (row 4 wave + r + dy, column l15 + dx)][plane g]
        f16x8 wf[2][2], xf[2][4];
        auto read_step = [&](const int tap, f16x8 (&w)[2], f16x8 (&x)[4]) {
          const int dy = tap / 3, dx = tap - 3 * dy;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int hp = (4 * wave + r + dy) * CD_HW + l15 + dx;
            x[r] = *reinterpret_cast<const f16x8*>(hb + g * CD_PLANE + ((hp ^ (2 * (g >> 1))) << 4));
          }
#pragma unroll
          for (int b = 0; b < 2; ++b) w[b] = *reinterpret_cast<const f16x8*>(wb + ((tap * 2 + b) * 64 + lane) * 16);
        };
        read_step(0, wf[0], xf[0]);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          if (k + 1 < 9) read_step(k + 1, wf[(k + 1) & 1], xf[(k + 1) & 1]);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[b][r] = mfma16x16x32(wf[k & 1][b], xf[k & 1][r], acc[b][r]);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (tn < ntiles) commit((it + 1) & 1);      // the other buffer was last read in iteration it - 1, closed by its barrier
        lds_barrier();                              // (LDS only: global stores stay in flight across it, common.h)
      }

      // ---- D[channel ch0 + 4 b + e][pixel l15] -> s2 (s1 lrelu(. + bias) + r1) + r2, 16 bytes per lane and store
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int64_t pix;
        if (locate(t, r, pix)) {      // (found again, not kept: four lane masks held across the MFMAs spill scalar registers)
          f16x8 o;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float v = acc[j >> 2][r][j & 3] + bv[j];
            v = v >= 0.f ? v : slope * v;
            if constexpr (WIDE) {
              v = s1 * v + (float)rr1[r][j];
              v = s2 * v + (float)rr2[r][j];
            }
            o[j] = (f16)v;
          }
          *reinterpret_cast<f16x8*>(O + pix * p.ldo + ch0) = o;
        }
      }
    }
  }
}

// bytes from the first to the last element of `c` channels of `pixels` pixels, `ld` elements apart
inline int64_t cd_span(const int64_t pixels, const int64_t ld, const int c) { return ((pixels - 1) * ld + c) * 2; }

// whether the channels [0, cb) of the pixels at b (stride ld) and the channels [0, ca) of the pixels at a (the same stride) are
// disjoint although the byte ranges overlap: a is b's buffer at a channel offset that leaves b's channels alone
inline bool cd_disjoint_channels(const void* a, const int ca, const void* b, const int cb, const int64_t ld) {
  const intptr_t d = (reinterpret_cast<intptr_t>(a) - reinterpret_cast<intptr_t>(b)) / 2;      // elements (both are 16-byte aligned)
  const int64_t c0 = ((d % ld) + ld) % ld;
  return c0 >= cb && c0 + ca <= ld;
}

}  // namespace

extern "C" int i2v_conv3x3_dense_f16(const i2v_conv_dense_params* p, i2v_stream_t stream) {
  const char* fn = "i2v_conv3x3_dense_f16";
  I2V_CHECK_ARG(p != nullptr, "%s: null params", fn);
  I2V_CHECK_ARG(p->x && p->w && p->out, "%s: null pointer", fn);
  I2V_CHECK_ARG(p->cin >= 64 && p->cin <= CD_MAXCIN && p->cin % 32 == 0, "%s: cin %d must be 64, 96, 128, 160 or 192", fn, p->cin);
  I2V_CHECK_ARG(p->cout == 32 || p->cout == 64, "%s: cout %d must be 32 or 64", fn, p->cout);
  I2V_CHECK_ARG(p->n_img >= 1 && p->height >= 1 && p->width >= 1, "%s: n %d, h %d, w %d", fn, p->n_img, p->height, p->width);
  const int64_t lim = (int64_t)1 << 31;
  I2V_CHECK_ARG(p->ldx >= p->cin && p->ldx % 8 == 0 && p->ldx < (1 << 20), "%s: pixel stride ldx %lld must be >= cin %d and a multiple of 8",
                fn, (long long)p->ldx, p->cin);
  I2V_CHECK_ARG(p->ldo >= p->cout && p->ldo % 8 == 0 && p->ldo < (1 << 20), "%s: pixel stride ldo %lld must be >= cout %d and a multiple of 8",
                fn, (long long)p->ldo, p->cout);
  I2V_CHECK_ARG(p->r1 == nullptr || (p->ldr1 >= p->cout && p->ldr1 % 8 == 0 && p->ldr1 < (1 << 20)),
                "%s: r1 pixel stride %lld must be >= cout %d and a multiple of 8", fn, (long long)p->ldr1, p->cout);
  I2V_CHECK_ARG(p->r2 == nullptr || (p->ldr2 >= p->cout && p->ldr2 % 8 == 0 && p->ldr2 < (1 << 20)),
                "%s: r2 pixel stride %lld must be >= cout %d and a multiple of 8", fn, (long long)p->ldr2, p->cout);
  I2V_CHECK_ARG(i2v_al16(p->x) && i2v_al16(p->w) && i2v_al16(p->out) && i2v_al16(p->bias) && i2v_al16(p->r1) && i2v_al16(p->r2),
                "%s: operands must be 16-byte aligned", fn);
  I2V_CHECK_ARG(p->slope == p->slope && p->s1 == p->s1 && p->s2 == p->s2, "%s: slope %g, s1 %g, s2 %g", fn, (double)p->slope, (double)p->s1,
                (double)p->s2);
  const int64_t hw = (int64_t)p->height * p->width, pixels = hw * p->n_img;
  I2V_CHECK_ARG(hw * p->ldx < lim && pixels < lim, "%s: problem too large", fn);
  const int64_t xb = cd_span(pixels, p->ldx, p->cin), ob = cd_span(pixels, p->ldo, p->cout);
  const int64_t wb = (int64_t)9 * p->cin * p->cout * 2;
  // other workgroups read channels < cin of x as halo while this one stores: out may share x's bytes only as OTHER channels of its pixels
  I2V_CHECK_ARG(!i2v_overlap(p->out, ob, p->x, xb) || (p->ldo == p->ldx && cd_disjoint_channels(p->out, p->cout, p->x, p->cin, p->ldx)),
                "%s: out overlaps channels 0..%d of x (other workgroups read them as halo)", fn, p->cin - 1);
  I2V_CHECK_ARG(!i2v_overlap(p->out, ob, p->w, wb) && (p->bias == nullptr || !i2v_overlap(p->out, ob, p->bias, p->cout * 2)),
                "%s: out overlaps the weights", fn);
  // every element of a residual is read by the lane that then stores it: out may BE a residual, and nothing in between
  I2V_CHECK_ARG(p->r1 == nullptr || (p->r1 == p->out && p->ldr1 == p->ldo) || !i2v_overlap(p->out, ob, p->r1, cd_span(pixels, p->ldr1, p->cout)),
                "%s: out overlaps r1 without being it", fn);
  I2V_CHECK_ARG(p->r2 == nullptr || (p->r2 == p->out && p->ldr2 == p->ldo) || !i2v_overlap(p->out, ob, p->r2, cd_span(pixels, p->ldr2, p->cout)),
                "%s: out overlaps r2 without being it", fn);
  I2V_CHECK_ARG(p->max_workgroups >= 0, "%s: max_workgroups %d", fn, p->max_workgroups);
  const int tiles_x = (int)i2v_cdiv(p->width, CD_TW), tiles_y = (int)i2v_cdiv(p->height, CD_TH);
  const int64_t ntiles = (int64_t)p->n_img * tiles_x * tiles_y;
  I2V_CHECK_ARG(ntiles < lim - (1 << 20), "%s: problem too large", fn);
  const bool wide = p->cout == 64 || p->r1 || p->r2 || p->s1 != 1.0f || p->s2 != 1.0f;
  const void* kernel = wide ? reinterpret_cast<const void*>(conv_dense_kernel<true>) : reinterpret_cast<const void*>(conv_dense_kernel<false>);
  const int cus = i2v_big_lds_kernel_cus(kernel, CD_LDS_MAX);
  if (cus <= 0) I2V_FAIL(I2V_ERR_UNSUPPORTED, "%s: the device refuses %d bytes of LDS", fn, CD_LDS_MAX);
  // a 64-channel output is two halves: two groups of workgroups, or one workgroup that walks the tiles twice
  const int nhalves = p->cout / 32;
  int64_t grid = p->max_workgroups > 0 ? p->max_workgroups : cus;
  if (grid > ntiles * nhalves) grid = ntiles * nhalves;
  const int groups = (nhalves == 2 && grid >= 2) ? 2 : 1;
  grid -= grid % groups;
  const int lds = p->cin / 32 * 9 * CD_WSTEP + 2 * CD_CHUNK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (wide)
    hipLaunchKernelGGL(conv_dense_kernel<true>, dim3((unsigned)grid), dim3(256), lds, st, *p, tiles_x, tiles_y, (int)ntiles, groups);
  else
    hipLaunchKernelGGL(conv_dense_kernel<false>, dim3((unsigned)grid), dim3(256), lds, st, *p, tiles_x, tiles_y, (int)ntiles, groups);
  return i2v_check_launch(fn);
}
