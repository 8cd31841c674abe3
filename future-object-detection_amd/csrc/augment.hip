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

}  // namespace

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
