// Device-side image half of the joint crop / resize / flip augmentation (reference future_od/datasets/transforms.py:
// BaseCrop 64-101, JointResize 41-61, JointHorizontalFlip 152-163), from the RAW uint8 frames to the normalised f32
// clip the model takes: one bilinear pass (align_corners = False, no antialiasing) over the crop rectangle, then the
// dataset's pixel pipeline ((v / 255) - mean) / std (transforms.py:12-15, nu_scenes.py:97-101) as stem_layout_kernel
// applies it.  Normalising after interpolating equals the reference's order (normalise, crop, resize): the four
// weights sum to one.
//
// A memory-bound gather: 4 output bytes per at most ~1 source byte.  One thread produces four consecutive x of one
// (b, l, y) row for all C planes -- the row / column indices and weights depend only on (y, x) -- and stores each
// plane's four values as one 16-byte store.  The source rows are byte loads; neighbouring threads read neighbouring
// bytes, and a crop that is smaller than the output re-reads them from L2.  No LDS, no atomics.
//
// fod_clip_crop_resize_photo (include/fod_ext.h) is the same pass with the colour half -- brightness, contrast,
// saturation and hue, one row per clip -- applied to the samples while they are in registers, before normalising.
//
// fod_clip_crop_resize_aa (include/fod_ext.h) is the ANTIALIASED pass: the same operands and pixel pipeline, every output
// the normalised triangle-filter average of its whole source footprint, separable through LDS (further down).
#include "common.h"
#include "../../include/fod_ext.h"

#include <algorithm>
#include <climits>

namespace {

struct CropRect {
  int top, left, height, width, flip;
};

// The plan row as the kernel uses it: a rectangle that leaves the frame is clamped INTO it (first its extent, then its
// origin), so whatever the device memory holds, every source index below lies inside the frame.
FOD_DEVINL CropRect load_rect(const int* __restrict__ p, int H0, int W0) {
  CropRect r;
  r.height = min(max(p[2], 1), H0);
  r.width = min(max(p[3], 1), W0);
  r.top = min(max(p[0], 0), H0 - r.height);
  r.left = min(max(p[1], 0), W0 - r.width);
  r.flip = p[4] != 0;
  return r;
}

// Source index pair and weight of output coordinate `o` (torch's area_pixel_compute_source_index, align_corners = False):
// s = max(scale * (o + 0.5) - 0.5, 0), i0 = floor(s), i1 = min(i0 + 1, extent - 1), both inside the crop rectangle.
FOD_DEVINL void source_index(float scale, int o, int extent, int& i0, int& i1, float& w) {
  const float s = fmaxf(scale * ((float)o + 0.5f) - 0.5f, 0.f);
  i0 = min((int)s, extent - 1);            // s >= 0: the cast is the floor
  i1 = min(i0 + 1, extent - 1);
  w = s - (float)i0;
}

__global__ __launch_bounds__(256) void clip_crop_resize_kernel(const unsigned char* __restrict__ src,
                                                               float* __restrict__ dst, int L, int C, int H0, int W0,
                                                               int H, int W, long src_stride_b, long src_stride_l,
                                                               const int* __restrict__ plans,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ stdv) {
  const int f = blockIdx.y;                 // frame b * L + l
  const int b = f / L;
  const CropRect r = load_rect(plans + 5 * b, H0, W0);
  const unsigned char* s = src + (long)b * src_stride_b + (long)(f - b * L) * src_stride_l + (long)r.top * W0 + r.left;
  float* o = dst + (long)f * C * H * W;
  const int hw0 = H0 * W0;
  const int hw = H * W;
  const float sy = (float)r.height / (float)H;
  const float sx = (float)r.width / (float)W;
  const bool vec = (W & 3) == 0;            // every output row starts 16-byte aligned
  const int groups = (W + 3) >> 2;
  const int n = H * groups;
  float m[3], sd[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {             // fully unrolled: the arrays stay in registers
    m[c] = c < C ? mean[c] : 0.f;
    sd[c] = c < C ? stdv[c] : 1.f;
  }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int y = i / groups;
    const int x = 4 * (i - y * groups);
    int y0, y1, x0[4], x1[4];
    float ly, lx[4];
    source_index(sy, y, r.height, y0, y1, ly);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xo = min(x + j, W - 1);     // the tail group repeats its last column; those lanes are not stored
      source_index(sx, r.flip ? W - 1 - xo : xo, r.width, x0[j], x1[j], lx[j]);
    }
    const unsigned char* r0 = s + y0 * W0;
    const unsigned char* r1 = s + y1 * W0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c < C) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float p00 = (float)r0[x0[j]], p01 = (float)r0[x1[j]];
          const float p10 = (float)r1[x0[j]], p11 = (float)r1[x1[j]];
          float val = (1.f - ly) * ((1.f - lx[j]) * p00 + lx[j] * p01) + ly * ((1.f - lx[j]) * p10 + lx[j] * p11);
          val = val / 255.f;
          v[j] = (val - m[c]) / sd[c];
        }
        float* q = o + c * hw + y * W + x;
        if (vec) {
          *reinterpret_cast<float4*>(q) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (x + j < W) q[j] = v[j];
        }
        r0 += hw0;
        r1 += hw0;
      }
    }
  }
}

// ---- the same pass with the photometric half (include/fod_ext.h, fod_clip_crop_resize_photo) --------------------------
// One row (delta, alpha, sat, hue, first) per clip, read from device memory and never trusted: a non-finite number
// becomes its neutral value, then delta -> [-1, 1], alpha and sat -> [0, 4], hue -> its fractional part.
struct PhotoRow {
  float delta, alpha, sat, hue;
  bool first, hsv, neutral;
};

FOD_DEVINL float finite_or(float v, float neutral) { return fabsf(v) <= 3.402823466e38f ? v : neutral; }   // NaN: false

FOD_DEVINL PhotoRow load_photo(const float* __restrict__ p) {
  PhotoRow r;
  r.delta = fminf(fmaxf(finite_or(p[0], 0.f), -1.f), 1.f);
  r.alpha = fminf(fmaxf(finite_or(p[1], 1.f), 0.f), 4.f);
  r.sat = fminf(fmaxf(finite_or(p[2], 1.f), 0.f), 4.f);
  const float hue = finite_or(p[3], 0.f);
  r.hue = hue - floorf(hue);
  r.first = !(p[4] == 0.f);
  r.hsv = r.sat != 1.f || r.hue != 0.f;
  r.neutral = r.delta == 0.f && r.alpha == 1.f && !r.hsv;
  return r;
}

FOD_DEVINL float unit(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// One channel of HSV -> RGB: v - v * s * max(0, min(k, 4 - k, 1)), k = fmod(n + 6h, 6).  n + 6h lies in [1, 12), where
// "subtract 6 once" IS fmod (the difference is exact).
FOD_DEVINL float hsv_channel(float n, float h, float v, float s) {
  const float t = n + 6.f * h;
  const float k = t >= 6.f ? t - 6.f : t;
  return v - v * s * fmaxf(0.f, fminf(fminf(k, 4.f - k), 1.f));
}

// Steps 1-5 of the header's definition on one pixel in 0..1; every branch on the row is uniform over the block.
FOD_DEVINL void photo_pixel(float& r, float& g, float& b, const PhotoRow& ph) {
  r += ph.delta; g += ph.delta; b += ph.delta;
  if (ph.first) { r *= ph.alpha; g *= ph.alpha; b *= ph.alpha; }
  if (ph.hsv) {
    r = unit(r); g = unit(g); b = unit(b);
    const float v = fmaxf(r, fmaxf(g, b)), m = fminf(r, fminf(g, b)), c = v - m;
    float s = 0.f, h6 = 0.f;
    if (c > 0.f) {                          // then v > 0 too
      s = c / v;
      if (v == r) {
        h6 = (g - b) / c;                   // in [-1, 1]: the non-negative fmod(., 6) adds 6 to a negative value
        h6 = h6 < 0.f ? h6 + 6.f : h6;
      } else if (v == g) {
        h6 = (b - r) / c + 2.f;
      } else {
        h6 = (r - g) / c + 4.f;
      }
    }
    s = fminf(s * ph.sat, 1.f);
    float h = h6 / 6.f + ph.hue;
    h -= floorf(h);
    r = hsv_channel(5.f, h, v, s);
    g = hsv_channel(3.f, h, v, s);
    b = hsv_channel(1.f, h, v, s);
  }
  if (!ph.first) { r *= ph.alpha; g *= ph.alpha; b *= ph.alpha; }
  r = unit(r); g = unit(g); b = unit(b);
}

// The geometry of clip_crop_resize_kernel for C == 3: a thread holds the three planes' samples of its four pixels (the
// photometric map mixes the planes), applies the clip's row to them, then normalises and stores as the parent does.
//
// A clip with a neutral row must come out with the parent's BITS, and the same expressions are not enough for that: the
// compiler contracts a * b + c * d into fma(a, b, c * d) or fma(c, d, a * b) as it sees fit, and in the parent it chose
// differently for neighbouring pixels of one thread (it pairs them into packed instructions).  So the neutral branch
// is the parent's loop, copied statement for statement, C a run-time argument as there (the entry point admits only 3):
// the same code in, the same instructions out.  tests/test_photometric_gpu.py holds the two kernels' bits together.
__global__ __launch_bounds__(256) void clip_crop_resize_photo_kernel(const unsigned char* __restrict__ src,
                                                                     float* __restrict__ dst, int L, int C, int H0,
                                                                     int W0, int H, int W, long src_stride_b,
                                                                     long src_stride_l,
                                                                     const int* __restrict__ plans,
                                                                     const float* __restrict__ mean,
                                                                     const float* __restrict__ stdv,
                                                                     const float* __restrict__ photo) {
  const int f = blockIdx.y;                 // frame b * L + l
  const int b = f / L;
  const CropRect r = load_rect(plans + 5 * b, H0, W0);
  const PhotoRow ph = load_photo(photo + 5 * b);
  const unsigned char* s = src + (long)b * src_stride_b + (long)(f - b * L) * src_stride_l + (long)r.top * W0 + r.left;
  float* o = dst + (long)f * C * H * W;
  const int hw0 = H0 * W0;
  const int hw = H * W;
  const float sy = (float)r.height / (float)H;
  const float sx = (float)r.width / (float)W;
  const bool vec = (W & 3) == 0;            // every output row starts 16-byte aligned
  const int groups = (W + 3) >> 2;
  const int n = H * groups;
  float m[3], sd[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {             // fully unrolled: the arrays stay in registers
    m[c] = c < C ? mean[c] : 0.f;
    sd[c] = c < C ? stdv[c] : 1.f;
  }
  if (ph.neutral) {                         // uniform over the block: clip_crop_resize_kernel's loop, see above
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
      const int y = i / groups;
      const int x = 4 * (i - y * groups);
      int y0, y1, x0[4], x1[4];
      float ly, lx[4];
      source_index(sy, y, r.height, y0, y1, ly);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int xo = min(x + j, W - 1);
        source_index(sx, r.flip ? W - 1 - xo : xo, r.width, x0[j], x1[j], lx[j]);
      }
      const unsigned char* r0 = s + y0 * W0;
      const unsigned char* r1 = s + y1 * W0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (c < C) {
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float p00 = (float)r0[x0[j]], p01 = (float)r0[x1[j]];
            const float p10 = (float)r1[x0[j]], p11 = (float)r1[x1[j]];
            float val = (1.f - ly) * ((1.f - lx[j]) * p00 + lx[j] * p01) + ly * ((1.f - lx[j]) * p10 + lx[j] * p11);
            val = val / 255.f;
            v[j] = (val - m[c]) / sd[c];
          }
          float* q = o + c * hw + y * W + x;
          if (vec) {
            *reinterpret_cast<float4*>(q) = make_float4(v[0], v[1], v[2], v[3]);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (x + j < W) q[j] = v[j];
          }
          r0 += hw0;
          r1 += hw0;
        }
      }
    }
    return;
  }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int y = i / groups;
    const int x = 4 * (i - y * groups);
    int y0, y1, x0[4], x1[4];
    float ly, lx[4];
    source_index(sy, y, r.height, y0, y1, ly);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xo = min(x + j, W - 1);     // the tail group repeats its last column; those lanes are not stored
      source_index(sx, r.flip ? W - 1 - xo : xo, r.width, x0[j], x1[j], lx[j]);
    }
    const unsigned char* r0 = s + y0 * W0;
    const unsigned char* r1 = s + y1 * W0;
    float v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p00 = (float)r0[x0[j]], p01 = (float)r0[x1[j]];
        const float p10 = (float)r1[x0[j]], p11 = (float)r1[x1[j]];
        float val = (1.f - ly) * ((1.f - lx[j]) * p00 + lx[j] * p01) + ly * ((1.f - lx[j]) * p10 + lx[j] * p11);
        v[c][j] = val / 255.f;
      }
      r0 += hw0;
      r1 += hw0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) photo_pixel(v[0][j], v[1][j], v[2][j], ph);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[c][j] = (v[c][j] - m[c]) / sd[c];
      float* q = o + c * hw + y * W + x;
      if (vec) {
        *reinterpret_cast<float4*>(q) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x + j < W) q[j] = v[c][j];
      }
    }
  }
}

// ---- the antialiased form (include/fod_ext.h, fod_clip_crop_resize_aa) --------------------------------------------------
// Separable, through LDS.  A workgroup of 256 owns an AA_TH x AA_TW output tile of one frame and walks the planes:
//   1. stage: the tile's source footprint of the plane, uint8 rows, global -> LDS as aligned dwords;
//   2. horizontal: thread (row r mod 4, column u) folds its column's taps of the staged rows into the f32 intermediate
//      [rows][AA_TW] -- the column's weights were formed once per tile and live in its registers;
//   3. vertical: thread (row y, four columns) folds its row's taps of the intermediate, read as float4, into registers.
// After the last plane a thread holds the three planes of its four pixels: the photometric row, if any, mixes them,
// then they are normalised and stored as 16 bytes per plane.
// LDS banks: a wave of the horizontal pass reads one staged row -- neighbouring lanes' taps lie `scale` bytes apart, at
// most 4, so 32 lanes span at most 32 dwords -- and writes 64 consecutive floats; in the vertical pass 16 lanes cover
// one 256-byte intermediate row, which is what each ds_read_b128 lane group needs to be conflict-free.
// The extents are sized for the ratio the entry point admits (AA_MAXR): a tile's footprint has at most
// (AA_TH - 1) * 4 + 2 * 4 + 1 rows and (AA_TW - 1) * 4 + 2 * 4 + 1 columns, and an output has fewer than 2 * 4 + 1 taps;
// the kernel still clamps every count and offset to what it staged.  The tap loops run to a bound that is uniform over
// the frame; an output with fewer taps has weight 0 there and multiplies it with whatever staged value lies at that place
// (a byte is always finite; the intermediate's row index is clamped, its unwritten rows could hold anything).
// What holds the kernel is pass 2 (profiles/antialias_kernel_rates.txt).
constexpr int AA_TH = 16, AA_TW = 64, AA_MAXR = 4;
constexpr int AA_TAPS = 2 * AA_MAXR + 2;
constexpr int AA_SR = AA_TH * AA_MAXR + 2 * AA_MAXR + 2;        // 74 rows
constexpr int AA_SC = AA_TW * AA_MAXR + 2 * AA_MAXR + 8;        // 272 bytes a row: 261 of footprint, 3 of alignment

// What ties the constants to the admitted ratio: with sup <= AA_MAXR an output has hi - lo < 2 * sup + 1 taps, that is at
// most ceil(2 * sup) <= 2 * AA_MAXR, plus one where the two f32 sums round apart; a tile's footprint is its last output's
// hi less its first output's lo.  Change AA_MAXR, the tile or the extents apart from each other and these fail.
static_assert(AA_TAPS >= 2 * AA_MAXR + 1, "an output's taps at the admitted ratio, rounding included");
static_assert(AA_SR >= (AA_TH - 1) * AA_MAXR + 2 * AA_MAXR + 2, "a tile's footprint rows at the admitted ratio");
static_assert(AA_SC - 4 >= (AA_TW - 1) * AA_MAXR + 2 * AA_MAXR + 2, "a tile's footprint columns, less the alignment bytes");
static_assert(AA_SC % 4 == 0 && AA_TW == 64 && AA_TH * (AA_TW / 4) == 256, "dword rows; the passes' thread maps");

// [lo, hi) of output index `o`: the header's definition, then clamped so that 0 <= lo < hi <= extent.
FOD_DEVINL void aa_span(float scale, float sup, int o, int extent, int& lo, int& hi) {
  const float c = __fmul_rn(scale, (float)o + 0.5f);
  lo = min(max((int)(c - sup + 0.5f), 0), extent - 1);
  hi = max(min((int)(c + sup + 0.5f), extent), lo + 1);
}

struct AaTaps {
  int lo;
  float w[AA_TAPS];                         // normalised; zero from the output's tap count on
};

FOD_DEVINL void aa_taps(float scale, float sup, int o, int extent, int cap, AaTaps& t) {
  const float c = __fmul_rn(scale, (float)o + 0.5f);
  int hi;
  aa_span(scale, sup, o, extent, t.lo, hi);
  // cap = min(AA_TAPS, ceil(2 * sup) + 1) is what the tap loops run to.  hi - lo < 2 * sup + 1 in exact arithmetic, so
  // hi - lo <= ceil(2 * sup), and one more at the most where c - sup + 0.5 and c + sup + 0.5 round apart: the min below
  // never cuts a tap off while sup <= AA_MAXR (the entry point's ratio check; the static_asserts above).  It is there
  // so that a count can never pass the registers it is held in.
  const int n = min(hi - t.lo, cap);
  const float inv = 1.f / sup;              // one division an axis: x / sup as x * (1 / sup), w / total likewise -- each
  float total = 0.f;                        // within an ulp of the quotient, and exact where sup or the sum is 1
#pragma unroll
  for (int k = 0; k < AA_TAPS; ++k) {
    t.w[k] = 0.f;
    if (k < cap) {                          // uniform over the frame
      const float w = k < n ? fmaxf(0.f, 1.f - fabsf(((float)(t.lo + k) - c + 0.5f) * inv)) : 0.f;
      t.w[k] = w;
      total += w;
    }
  }
  if (total != 0.f) {
    const float scale_w = 1.f / total;
#pragma unroll
    for (int k = 0; k < AA_TAPS; ++k) t.w[k] *= scale_w;
  }
}

__global__ __launch_bounds__(256) void clip_crop_resize_aa_kernel(const unsigned char* __restrict__ src,
                                                                  float* __restrict__ dst, int L, int C, int H0, int W0,
                                                                  int H, int W, long src_stride_b, long src_stride_l,
                                                                  const int* __restrict__ plans,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ stdv,
                                                                  const float* __restrict__ photo) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[AA_SR * AA_SC + 16];      // + a zero-weight tap's reach
  __shared__ __attribute__((aligned(16))) float inter[AA_SR * AA_TW];
  const int f = blockIdx.y;                 // frame b * L + l
  const int b = f / L;
  const CropRect r = load_rect(plans + 5 * b, H0, W0);
  PhotoRow ph = {};
  bool mix = false;
  if (photo) {                              // uniform over the block
    ph = load_photo(photo + 5 * b);
    mix = !ph.neutral;
  }
  const int hw0 = H0 * W0;
  const int hw = H * W;
  const unsigned char* frame = src + (long)b * src_stride_b + (long)(f - b * L) * src_stride_l;
  const unsigned char* frame_end = frame + (long)C * hw0;
  const unsigned char* s = frame + (long)r.top * W0 + r.left;
  float* o = dst + (long)f * C * H * W;
  const float sy = (float)r.height / (float)H, supy = fmaxf(sy, 1.f);
  const float sx = (float)r.width / (float)W, supx = fmaxf(sx, 1.f);
  const int capy = min(AA_TAPS, (int)ceilf(2.f * supy) + 1);      // fewer than 2 * sup + 1 taps: uniform over the frame
  const int capx = min(AA_TAPS, (int)ceilf(2.f * supx) + 1);
  const int tiles_x = (W + AA_TW - 1) / AA_TW;
  const int y0 = (blockIdx.x / tiles_x) * AA_TH;
  const int u0 = (blockIdx.x % tiles_x) * AA_TW;                  // u: the column before the flip
  // the tile's footprint inside the rectangle: lo and hi do not decrease with the output index
  int row0, rowe, col0, cole, unused;
  aa_span(sy, supy, y0, r.height, row0, unused);
  aa_span(sy, supy, min(y0 + AA_TH, H) - 1, r.height, unused, rowe);
  aa_span(sx, supx, u0, r.width, col0, unused);
  aa_span(sx, supx, min(u0 + AA_TW, W) - 1, r.width, unused, cole);
  const int nrows = min(rowe - row0, AA_SR);
  const int ncols = min(cole - col0, AA_SC - 4);                  // + up to 3 bytes of alignment in front
  const int ndmax = (ncols + 6) >> 2;                             // dwords a staged row can take
  const int total = nrows * ndmax;
  const float inv_nd = 1.f / (float)ndmax;
  const int tid = threadIdx.x;
  const int hr = tid >> 6, hx = tid & 63;   // horizontal pass: rows hr, hr + 4, ... of column u0 + hx; hr is the wave
  const int vy = tid >> 4, vx = (tid & 15) * 4;                   // vertical pass: row y0 + vy, columns u0 + vx .. + 3
  AaTaps tx, ty;
  aa_taps(sx, supx, min(u0 + hx, W - 1), r.width, capx, tx);      // past the edge: the last column again, not stored
  aa_taps(sy, supy, min(y0 + vy, H - 1), r.height, capy, ty);
  const int offx = min(max(tx.lo - col0, 0), ncols - 1);
  const int offy = min(max(ty.lo - row0, 0), nrows - 1);
  float m[3], sd[3], v[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c) {             // fully unrolled: the arrays stay in registers
    m[c] = c < C ? mean[c] : 0.f;
    sd[c] = c < C ? stdv[c] : 1.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[c][j] = 0.f;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (c < C) {                            // uniform: the barriers below are reached by all or none
      // Stage: whole ALIGNED dwords, four requests in flight per thread.  A staged row starts at the aligned address at
      // or below its first byte, so its pixels begin `row address & 3` bytes in (the horizontal pass adds that back).
      // A dword that is not wholly inside the frame's planes -- only the first or the last of a frame can be -- is
      // put together from the bytes that are.
      const unsigned char* p = s + (long)c * hw0 + (long)row0 * W0 + col0;
      for (int i0 = tid; i0 < total; i0 += 4 * 256) {
        unsigned int word[4];
        int at[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = i0 + 256 * q;
          at[q] = -1;
          if (i < total) {
            int rr = (int)((float)i * inv_nd);            // i / ndmax without the integer division: i < 2^13, so
            rr -= rr * ndmax > i;                         // the float quotient is off by one at the most
            rr += (rr + 1) * ndmax <= i;
            const int d = i - rr * ndmax;
            const unsigned char* rowp = p + rr * W0;
            const int lead = (int)((uintptr_t)rowp & 3);
            if (4 * d < lead + ncols) {
              const unsigned char* a = rowp - lead + 4 * d;
              at[q] = rr * (AA_SC / 4) + d;
              if (a >= frame && a + 4 <= frame_end) {
                word[q] = *reinterpret_cast<const unsigned int*>(a);
              } else {
                word[q] = 0;
#pragma unroll
                for (int t = 0; t < 4; ++t)
                  if (a + t >= frame && a + t < frame_end) word[q] |= (unsigned int)a[t] << (8 * t);
              }
            }
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (at[q] >= 0) reinterpret_cast<unsigned int*>(stage)[at[q]] = word[q];
      }
      __syncthreads();
      for (int rr = hr; rr < nrows; rr += 4) {
        const int lead = (int)((uintptr_t)(p + rr * W0) & 3);
        const unsigned char* q = stage + rr * AA_SC + lead + offx;
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < AA_TAPS; ++k)
          if (k < capx) a += tx.w[k] * (float)q[k];       // past the column's taps: weight 0 times some staged byte
        inter[rr * AA_TW + hx] = a;
      }
      __syncthreads();                      // the next plane's stage may now be written; its barrier guards `inter`
      float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < AA_TAPS; ++k)
        if (k < capy) {
          const float4 t = *reinterpret_cast<const float4*>(inter + min(offy + k, nrows - 1) * AA_TW + vx);
          a[0] += ty.w[k] * t.x;
          a[1] += ty.w[k] * t.y;
          a[2] += ty.w[k] * t.z;
          a[3] += ty.w[k] * t.w;
        }
#pragma unroll
      for (int j = 0; j < 4; ++j) v[c][j] = a[j] / 255.f;
    }
  }
  if (mix) {
#pragma unroll
    for (int j = 0; j < 4; ++j) photo_pixel(v[0][j], v[1][j], v[2][j], ph);
  }
  const int y = y0 + vy, u = u0 + vx;
  if (y >= H || u >= W) return;
  const bool vec = (W & 3) == 0;            // every output row starts 16-byte aligned, and u + 3 < W
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (c < C) {
      float e[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = (v[c][j] - m[c]) / sd[c];
      float* q = o + c * hw + y * W;
      if (vec) {
        if (r.flip) *reinterpret_cast<float4*>(q + (W - 4 - u)) = make_float4(e[3], e[2], e[1], e[0]);
        else *reinterpret_cast<float4*>(q + u) = make_float4(e[0], e[1], e[2], e[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (u + j < W) q[r.flip ? W - 1 - (u + j) : u + j] = e[j];
      }
    }
  }
}

}  // namespace

extern "C" int fod_clip_crop_resize_aa(const unsigned char* src, float* dst, int B, int L, int C, int H0, int W0, int H,
                                       int W, long src_stride_b, long src_stride_l, const int* plans, const float* mean,
                                       const float* stdv, const float* photo, hipStream_t stream) {
  FOD_REQUIRE(src && dst && plans && mean && stdv, "clip_crop_resize_aa: null pointer");
  FOD_REQUIRE(B > 0 && L > 0 && (long)B * L <= 65535 && C > 0 && C <= 3, "clip_crop_resize_aa: bad clip extent %dx%dx%d", B,
              L, C);
  FOD_REQUIRE(!photo || C == 3, "clip_crop_resize_aa: the photometric map mixes three planes, got C = %d", C);
  FOD_REQUIRE(H0 > 0 && W0 > 0 && (long)C * H0 * W0 <= INT_MAX, "clip_crop_resize_aa: bad source frame %dx%d", H0, W0);
  FOD_REQUIRE(H > 0 && W > 0 && (long)C * H * (W + 3) <= INT_MAX, "clip_crop_resize_aa: bad output frame %dx%d", H, W);
  FOD_REQUIRE(H0 <= (long)AA_MAXR * H && W0 <= (long)AA_MAXR * W,
              "clip_crop_resize_aa: a %dx%d frame is more than %d times the %dx%d output on an axis (the tile's LDS "
              "footprint is sized for that ratio)", H0, W0, AA_MAXR, H, W);
  FOD_REQUIRE(src_stride_l >= (long)C * H0 * W0 && src_stride_b >= (long)C * H0 * W0,
              "clip_crop_resize_aa: frame strides %ld / %ld overlap the %dx%dx%d planes", src_stride_b, src_stride_l, C,
              H0, W0);
  FOD_REQUIRE(((uintptr_t)dst % 16) == 0, "clip_crop_resize_aa: destination must be 16-byte aligned");
  const long tiles = (long)((H + AA_TH - 1) / AA_TH) * ((W + AA_TW - 1) / AA_TW);
  FOD_REQUIRE(tiles <= INT_MAX, "clip_crop_resize_aa: %ld tiles a frame", tiles);
  hipLaunchKernelGGL(clip_crop_resize_aa_kernel, dim3((unsigned)tiles, B * L), dim3(256), 0, stream, src, dst, L, C, H0,
                     W0, H, W, src_stride_b, src_stride_l, plans, mean, stdv, photo);
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}

extern "C" int fod_clip_crop_resize_photo(const unsigned char* src, float* dst, int B, int L, int C, int H0, int W0,
                                          int H, int W, long src_stride_b, long src_stride_l, const int* plans,
                                          const float* mean, const float* stdv, const float* photo, hipStream_t stream) {
  FOD_REQUIRE(src && dst && plans && mean && stdv && photo, "clip_crop_resize_photo: null pointer");
  FOD_REQUIRE(C == 3, "clip_crop_resize_photo: the photometric map mixes three planes, got C = %d", C);
  FOD_REQUIRE(B > 0 && L > 0 && (long)B * L <= 65535, "clip_crop_resize_photo: bad clip extent %dx%dx%d", B, L, C);
  FOD_REQUIRE(H0 > 0 && W0 > 0 && (long)C * H0 * W0 <= INT_MAX, "clip_crop_resize_photo: bad source frame %dx%d", H0, W0);
  FOD_REQUIRE(H > 0 && W > 0 && (long)C * H * (W + 3) <= INT_MAX, "clip_crop_resize_photo: bad output frame %dx%d", H, W);
  FOD_REQUIRE(src_stride_l >= (long)C * H0 * W0 && src_stride_b >= (long)C * H0 * W0,
              "clip_crop_resize_photo: frame strides %ld / %ld overlap the %dx%dx%d planes", src_stride_b, src_stride_l,
              C, H0, W0);
  FOD_REQUIRE(((uintptr_t)dst % 16) == 0, "clip_crop_resize_photo: destination must be 16-byte aligned");
  const long n = (long)H * ((W + 3) / 4);
  const int bx = (int)std::min<long>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(clip_crop_resize_photo_kernel, dim3(bx, B * L), dim3(256), 0, stream, src, dst, L, C, H0, W0, H, W,
                     src_stride_b, src_stride_l, plans, mean, stdv, photo);
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}

extern "C" int fod_clip_crop_resize(const unsigned char* src, float* dst, int B, int L, int C, int H0, int W0, int H,
                                    int W, long src_stride_b, long src_stride_l, const int* plans, const float* mean,
                                    const float* stdv, hipStream_t stream) {
  FOD_REQUIRE(src && dst && plans && mean && stdv, "clip_crop_resize: null pointer");
  FOD_REQUIRE(B > 0 && L > 0 && (long)B * L <= 65535 && C > 0 && C <= 3, "clip_crop_resize: bad clip extent %dx%dx%d", B,
              L, C);
  FOD_REQUIRE(H0 > 0 && W0 > 0 && (long)C * H0 * W0 <= INT_MAX, "clip_crop_resize: bad source frame %dx%d", H0, W0);
  FOD_REQUIRE(H > 0 && W > 0 && (long)C * H * (W + 3) <= INT_MAX, "clip_crop_resize: bad output frame %dx%d", H, W);
  FOD_REQUIRE(src_stride_l >= (long)C * H0 * W0 && src_stride_b >= (long)C * H0 * W0,
              "clip_crop_resize: frame strides %ld / %ld overlap the %dx%dx%d planes", src_stride_b, src_stride_l, C, H0,
              W0);
  FOD_REQUIRE(((uintptr_t)dst % 16) == 0, "clip_crop_resize: destination must be 16-byte aligned");
  const long n = (long)H * ((W + 3) / 4);
  const int bx = (int)std::min<long>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(clip_crop_resize_kernel, dim3(bx, B * L), dim3(256), 0, stream, src, dst, L, C, H0, W0, H, W,
                     src_stride_b, src_stride_l, plans, mean, stdv);
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}
