// Visualisation (reference future_od/utils/visualization.py: revert_imagenet_normalization, draw_boxes, the `* 255` and
// `.byte()` of visualize): one frame per sample of a clip becomes an 8-bit interleaved RGB picture with box outlines
// painted on it, in ONE launch.  include/fod_ext.h (fod_render_boxes) states the map; future_od/utils/visualization.py
// (draw_boxes) is its CPU form.
//
// Memory-bound when few boxes reach a pixel: 12 B read (f32) or 3 B (uint8) and 3 B written per pixel.  A block owns a
// tile of RB_TILE_H rows x RB_TILE_W pixels.  It first stages the sample's boxes into LDS -- the four integer edges and
// the packed colour, in index order, without the boxes that are not drawn and (RB_CULL) without those whose bars cannot
// reach the tile -- then every thread produces four consecutive pixels of a row: one 16-byte load per plane, the staged
// boxes scanned from the last to the first until each pixel has its colour (the painter's order: the highest index
// wins), twelve bytes out as three dword stores.  A wave is one row of the tile, so a box's row tests are wave-uniform
// and the LDS reads are broadcasts.  Rows whose addresses are not aligned, and the W % 4 tail, go element by element.
// No atomics, no traffic between blocks, every output byte written by exactly one thread.
// fod_render_attention (the maps of a detection over their frames) and fod_render_labels (captions on the pictures
// of fod_render_boxes) follow further down with the same tiles.
#include "common.h"
#include "../../include/fod_ext.h"

#include <climits>

// 1: boxes whose bars miss the block's tile are not staged.  Measured (profiles/render_boxes_cost.txt); the product
// build keeps the faster form, tools/measure_render.py builds the other one beside it.
#ifndef RB_CULL
#define RB_CULL 1
#endif

namespace {

constexpr int RB_THREADS = 256;
constexpr int RB_WAVES = RB_THREADS / 64;
constexpr int RB_TILE_W = 64 * 4;           // one wave, four pixels per lane
constexpr int RB_TILE_H = 16;               // RB_WAVES rows at a time
constexpr int RB_MAX_BOXES = 1024;          // the matcher's query limit

// v = x * std + mean, then v * 255: three roundings, no fused multiply-add.  Truncated towards zero and clamped to
// 0..255; a value that is not finite gives 0.  The pragma keeps the product and the sum apart (optim.hip, ema_step:
// hipcc's default contraction fuses them otherwise, and a float32 restatement then differs at the truncation).
FOD_DEVINL unsigned to_byte(float x, float sd, float m) {
#pragma clang fp contract(off)
  const float v = x * sd;
  const float u = v + m;
  const float w = u * 255.f;
  if (!(fabsf(w) <= 3.402823466e38f)) return 0u;            // NaN: false
  return (unsigned)fminf(fmaxf(w, 0.f), 255.f);              // in range: the cast truncates
}
FOD_DEVINL unsigned to_byte(unsigned char x, float, float) { return x; }

FOD_DEVINL int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Bit j set iff column x + j lies in [lo, hi), j = 0..3: the bits from clamp(lo - x) up to clamp(hi - x).  An empty or
// reversed range gives 0.
FOD_DEVINL unsigned columns(int x, int lo, int hi) {
  const int a = min(max(lo - x, 0), 4), b = min(max(hi - x, 0), 4);
  return ((1u << b) - 1u) & ~((1u << a) - 1u);
}

template <typename T>
struct Quad;                                 // four consecutive elements of a plane in one load
template <>
struct Quad<float> {
  float4 v;
  FOD_DEVINL void load(const float* p) { v = *reinterpret_cast<const float4*>(p); }
  FOD_DEVINL float at(int j) const { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
  static constexpr unsigned ALIGN = 16;
};
template <>
struct Quad<unsigned char> {
  unsigned v;
  FOD_DEVINL void load(const unsigned char* p) { v = *reinterpret_cast<const unsigned*>(p); }
  FOD_DEVINL unsigned char at(int j) const { return (unsigned char)(v >> (8 * j)); }
  static constexpr unsigned ALIGN = 4;
};

template <typename T>
__global__ __launch_bounds__(RB_THREADS) void render_boxes_kernel(const T* __restrict__ src,
                                                                  unsigned char* __restrict__ dst, int L, int H, int W,
                                                                  long src_stride_b, long src_stride_l,
                                                                  const int* __restrict__ frame_idx,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ stdv,
                                                                  const float* __restrict__ boxes,
                                                                  const int* __restrict__ labels, int N,
                                                                  const unsigned char* __restrict__ palette, int P,
                                                                  int t) {
  __shared__ int4 s_edge[RB_MAX_BOXES];      // (Lf, Tp, Rt, Bt)
  __shared__ unsigned s_colour[RB_MAX_BOXES];
  __shared__ int s_count[RB_WAVES];
  const int b = blockIdx.z;
  const int tx0 = blockIdx.x * RB_TILE_W, ty0 = blockIdx.y * RB_TILE_H;
  const int lane = threadIdx.x & 63, wave = uniform((int)threadIdx.x >> 6);

  // ---- stage the sample's boxes: index order is kept, so the scan below sees the painter's order
  int staged = 0;                            // the same in every thread
  const float lo = (float)t, hx = (float)(W - t), hy = (float)(H - t);
  for (int base = 0; base < N; base += RB_THREADS) {
    const int i = base + (int)threadIdx.x;
    bool keep = false;
    int4 e = make_int4(0, 0, 0, 0);
    unsigned colour = 0;
    if (i < N) {
      const int label = labels[(long)b * N + i];
      const float* q = boxes + ((long)b * N + i) * 4;
      const float x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3];
      if (label >= 0 && label < P && x1 == x1 && y1 == y1 && x2 == x2 && y2 == y2) {
        e.x = (int)fminf(fmaxf(x1, lo), hx);
        e.y = (int)fminf(fmaxf(y1, lo), hy);
        e.z = (int)fminf(fmaxf(x2, lo), hx);
        e.w = (int)fminf(fmaxf(y2, lo), hy);
        const unsigned char* c = palette + 3 * label;
        colour = (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16);
        keep = true;
#if RB_CULL
        // the bars lie inside [min - t, max + t) of the two edges in each direction (a reversed box has max < min of
        // the plain order: its remaining bars still lie in this range)
        keep = min(e.x, e.z) - t < tx0 + RB_TILE_W && max(e.x, e.z) + t > tx0 &&
               min(e.y, e.w) - t < ty0 + RB_TILE_H && max(e.y, e.w) + t > ty0;
#endif
      }
    }
    const unsigned long long votes = __ballot(keep);
    if (lane == 0) s_count[wave] = __popcll(votes);
    __syncthreads();
    int at = staged, total = 0;
#pragma unroll
    for (int w = 0; w < RB_WAVES; ++w) {
      if (w < wave) at += s_count[w];
      total += s_count[w];
    }
    if (keep) {
      at += __popcll(votes & ((1ull << lane) - 1ull));
      s_edge[at] = e;
      s_colour[at] = colour;
    }
    staged += total;
    __syncthreads();                         // the counts are rewritten next round; after the last, the stage is whole
  }

  // ---- the picture
  int f = frame_idx ? frame_idx[b] : 0;
  if (f < 0) f += L;
  f = min(max(f, 0), L - 1);
  const T* frame = src + (long)b * src_stride_b + (long)f * src_stride_l;
  const long hw = (long)H * W;
  float m[3] = {0.f, 0.f, 0.f}, sd[3] = {1.f, 1.f, 1.f};
  if (mean && stdv) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      m[c] = mean[c];
      sd[c] = stdv[c];
    }
  }
  const int x = tx0 + 4 * lane;
  if (x >= W) return;                        // (after the last barrier)
  for (int y = ty0 + wave; y < min(ty0 + RB_TILE_H, H); y += RB_WAVES) {
    const T* p = frame + (long)y * W + x;
    unsigned char* o = dst + (((long)b * H + y) * W + x) * 3;
    const bool whole = x + 3 < W;
    const bool aligned = whole && (((uintptr_t)p | (uintptr_t)(p + hw) | (uintptr_t)(p + 2 * hw)) % Quad<T>::ALIGN) == 0;
    Quad<T> q[3] = {};
    if (aligned) {                           // issued before the scan: the loads fly while the boxes are tested
#pragma unroll
      for (int c = 0; c < 3; ++c) q[c].load(p + c * hw);
    }
    unsigned px[4] = {0u, 0u, 0u, 0u};
    unsigned done = whole ? 0u : (0xFu << (W - x)) & 0xFu;  // bit j: pixel x + j has its colour (or lies past the row)
    // y, k and what s_edge[k] holds are the same in every lane of the wave: the row tests and the bars' extents are
    // scalar work (readfirstlane says so to the compiler), a lane only places its four pixels in a bar's columns
    for (int k = staged - 1; k >= 0; --k) {
      if (__ballot(done != 0xFu) == 0) break;               // every pixel of the wave's row has met its topmost box
      const int4 e = s_edge[k];
      const int lf = uniform(e.x), tp = uniform(e.y), rt = uniform(e.z), bt = uniform(e.w);
      const bool left = y >= tp - t && y < bt, bottom = y >= bt && y < bt + t;
      const bool right = y >= tp && y < bt + t, top = y >= tp - t && y < tp;
      if (!(left || bottom || right || top)) continue;
      unsigned hit = 0u;
      if (left) hit |= columns(x, lf - t, lf);
      if (bottom) hit |= columns(x, lf - t, rt);
      if (right) hit |= columns(x, rt, rt + t);
      if (top) hit |= columns(x, lf, rt + t);
      const unsigned fresh = hit & ~done;
      const unsigned colour = (unsigned)uniform((int)s_colour[k]);
#pragma unroll
      for (int j = 0; j < 4; ++j) px[j] = (fresh >> j & 1u) ? colour : px[j];
      done |= hit;
    }
    const unsigned painted = done;
    if (aligned) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (!(painted >> j & 1u))
          px[j] = to_byte(q[0].at(j), sd[0], m[0]) | (to_byte(q[1].at(j), sd[1], m[1]) << 8) |
                  (to_byte(q[2].at(j), sd[2], m[2]) << 16);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x + j < W && !(painted >> j & 1u))
          px[j] = to_byte(p[j], sd[0], m[0]) | (to_byte(p[hw + j], sd[1], m[1]) << 8) |
                  (to_byte(p[2 * hw + j], sd[2], m[2]) << 16);
    }
    if (whole && ((uintptr_t)o & 3u) == 0) {
      unsigned* o4 = reinterpret_cast<unsigned*>(o);         // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
      o4[0] = px[0] | (px[1] << 24);
      o4[1] = (px[1] >> 8) | (px[2] << 16);
      o4[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x + j < W) {
          o[3 * j] = (unsigned char)px[j];
          o[3 * j + 1] = (unsigned char)(px[j] >> 8);
          o[3 * j + 2] = (unsigned char)(px[j] >> 16);
        }
    }
  }
}

// ---- attention overlay (fod_render_attention): the maps of one detection per sample blended over their past frames.
// One launch for all B x J pictures; a thread produces four consecutive pixels of a row, as above.  The small map is
// sampled bilinearly from global memory (a 29x50 map is 5.8 KB: cache hits), the colour table is staged in LDS.

struct Tap {                                 // the two source rows (columns) of a destination row (column) and their weights
  int i0, i1;
  float w0, w1;
};
// F.interpolate's bilinear source coordinate with align_corners=False, every step one f32 operation
FOD_DEVINL Tap tap(int d, float ratio, int n) {
#pragma clang fp contract(off)
  float f = (float)d + 0.5f;
  f = f * ratio;
  f = f - 0.5f;
  f = fmaxf(f, 0.f);
  Tap t;
  t.i0 = min((int)f, n - 1);
  t.i1 = min(t.i0 + 1, n - 1);
  t.w1 = f - (float)t.i0;
  t.w0 = 1.f - t.w1;
  return t;
}

// background byte bg under the map sample a -> the blended byte of one channel; colour is the table's byte
FOD_DEVINL unsigned blend(unsigned bg, unsigned colour, float alpha) {
#pragma clang fp contract(off)
  const float keep = 1.f - alpha;
  const float u = (float)bg * keep;
  const float v = (float)colour * alpha;
  const float w = u + v;
  return (unsigned)fminf(fmaxf(w, 0.f), 255.f);
}

template <typename T>
__global__ __launch_bounds__(RB_THREADS) void render_attention_kernel(
    const T* __restrict__ src, unsigned char* __restrict__ dst, int L, int J, int H, int W, long src_stride_b,
    long src_stride_l, const int* __restrict__ frame_idx, const float* __restrict__ mean, const float* __restrict__ stdv,
    const float* __restrict__ maps, int h, int w, long map_stride_b, long map_stride_j,
    const float* __restrict__ colour_scale, const unsigned char* __restrict__ lut, float gain, float max_alpha) {
#pragma clang fp contract(off)
  __shared__ unsigned s_lut[256];
  {
    const unsigned char* c = lut + 3 * threadIdx.x;          // RB_THREADS == 256 entries
    s_lut[threadIdx.x] = (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16);
  }
  __syncthreads();
  const int b = blockIdx.z / J, j = blockIdx.z - b * J;
  const int tx0 = blockIdx.x * RB_TILE_W, ty0 = blockIdx.y * RB_TILE_H;
  const int lane = threadIdx.x & 63, wave = uniform((int)threadIdx.x >> 6);
  int f = frame_idx[b * J + j];
  if (f < 0) f += L;
  f = min(max(f, 0), L - 1);
  const T* frame = src + (long)b * src_stride_b + (long)f * src_stride_l;
  const float* map = maps + (long)b * map_stride_b + (long)j * map_stride_j;
  const float cs = colour_scale[b * J + j];
  const long hw = (long)H * W;
  float m[3] = {0.f, 0.f, 0.f}, sd[3] = {1.f, 1.f, 1.f};
  if (mean && stdv) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      m[c] = mean[c];
      sd[c] = stdv[c];
    }
  }
  const float ry = (float)h / (float)H, rx = (float)w / (float)W;
  const int x = tx0 + 4 * lane;
  if (x >= W) return;                        // (after the barrier)
  Tap cx[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) cx[k] = tap(min(x + k, W - 1), rx, w);
  for (int y = ty0 + wave; y < min(ty0 + RB_TILE_H, H); y += RB_WAVES) {
    const T* p = frame + (long)y * W + x;
    unsigned char* o = dst + ((((long)b * J + j) * H + y) * W + x) * 3;
    const bool whole = x + 3 < W;
    const bool aligned = whole && (((uintptr_t)p | (uintptr_t)(p + hw) | (uintptr_t)(p + 2 * hw)) % Quad<T>::ALIGN) == 0;
    Quad<T> q[3] = {};
    if (aligned) {
#pragma unroll
      for (int c = 0; c < 3; ++c) q[c].load(p + c * hw);
    }
    const Tap cy = tap(y, ry, h);
    const float* r0 = map + (long)cy.i0 * w;
    const float* r1 = map + (long)cy.i1 * w;
    unsigned px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (x + k >= W) continue;
      unsigned bg[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) bg[c] = aligned ? to_byte(q[c].at(k), sd[c], m[c]) : to_byte(p[c * hw + k], sd[c], m[c]);
      const float t0 = r0[cx[k].i0] * cx[k].w0, t1 = r0[cx[k].i1] * cx[k].w1, top = t0 + t1;
      const float u0 = r1[cx[k].i0] * cx[k].w0, u1 = r1[cx[k].i1] * cx[k].w1, bot = u0 + u1;
      const float a0 = top * cy.w0, a1 = bot * cy.w1, a = a0 + a1;
      if (fabsf(a) <= 3.402823466e38f) {                     // NaN or +-inf: the background stays
        float al = a * gain;
        al = al >= 0.f ? al : 0.f;                            // (a NaN product counts as 0)
        al = fminf(al, max_alpha);
        float ci = a * cs;
        ci = ci >= 0.f ? ci : 0.f;
        ci = fminf(ci, 1.f);
        ci = ci * 255.f;
        const unsigned colour = s_lut[(int)ci];
#pragma unroll
        for (int c = 0; c < 3; ++c) bg[c] = blend(bg[c], colour >> (8 * c) & 255u, al);
      }
      px[k] = bg[0] | (bg[1] << 8) | (bg[2] << 16);
    }
    if (whole && ((uintptr_t)o & 3u) == 0) {
      unsigned* o4 = reinterpret_cast<unsigned*>(o);         // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
      o4[0] = px[0] | (px[1] << 24);
      o4[1] = (px[1] >> 8) | (px[2] << 16);
      o4[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x + k < W) {
          o[3 * k] = (unsigned char)px[k];
          o[3 * k + 1] = (unsigned char)(px[k] >> 8);
          o[3 * k + 2] = (unsigned char)(px[k] >> 16);
        }
    }
  }
}

// ---- captions (fod_render_labels): index, class name and score of every drawn box as text on a plate above it, in
// place on the pictures fod_render_boxes wrote.  Built as render_boxes_kernel is: a block owns the same tile, stages
// the labels whose plates reach it -- rectangle, colours and the composed characters, in index order -- and every
// thread then decides four consecutive pixels of a row, scanning the staged labels from the last to the first until
// each pixel has met its topmost plate.  A wave is one row, so a plate's row test and its glyph row are wave-uniform;
// a lane divides its column into (character, glyph column) and reads one character and one font byte from LDS.
// Pixels outside every plate are neither read nor written; a painted pixel has exactly one writer.
constexpr int RL_MAX_CHARS = 32;             // FOD_LABEL_MAX_CHARS of the header
constexpr int RL_FONT_BYTES = 256 * 16;      // at most 256 glyphs of at most 16 rows

__global__ __launch_bounds__(RB_THREADS) void render_labels_kernel(
    unsigned char* __restrict__ dst, int H, int W, const float* __restrict__ boxes, const int* __restrict__ labels, int N,
    const int* __restrict__ idents, const float* __restrict__ scores, const unsigned char* __restrict__ names,
    int n_names, int name_stride, const unsigned char* __restrict__ palette, int P,
    const unsigned char* __restrict__ font, int font_first, int G, int FW, int FH, int s, int t) {
  __shared__ int4 s_rect[RB_MAX_BOXES];      // (x0, y0, x1, y1): the plate's corner and its clipped end
  __shared__ unsigned s_colour[RB_MAX_BOXES];                  // plate colour, bit 24: white ink
  __shared__ unsigned char s_text[RB_MAX_BOXES * RL_MAX_CHARS];
  __shared__ unsigned char s_font[RL_FONT_BYTES];
  __shared__ int s_count[RB_WAVES];
  const int b = blockIdx.z;
  const int tx0 = blockIdx.x * RB_TILE_W, ty0 = blockIdx.y * RB_TILE_H;
  const int lane = threadIdx.x & 63, wave = uniform((int)threadIdx.x >> 6);
  const int cw = FW + 1, Hp = (FH + 2) * s;
  // a / d as (a * (65536 / d + 1)) >> 16: exact for d <= 9 and a < 7273, and no plate is wider than 2312 pixels or has
  // more than 288 font columns (the division the compiler writes for an unknown d is some thirty instructions, three
  // times per pixel, in a kernel that waits on its own results: 36.7 -> 29.4 us at 300 captions)
  const unsigned by_s = 65536u / (unsigned)s + 1u, by_cw = 65536u / (unsigned)cw + 1u;

  for (int i = (int)threadIdx.x; i < G * FH; i += RB_THREADS) s_font[i] = font[i];

  // ---- stage the labels whose plates reach the tile, in index order
  int staged = 0;                            // the same in every thread
  const float lo = (float)t, hx = (float)(W - t), hy = (float)(H - t);
  for (int base = 0; base < N; base += RB_THREADS) {
    const int i = base + (int)threadIdx.x;
    bool keep = false;
    int4 r = make_int4(0, 0, 0, 0);
    unsigned colour = 0;
    int ident = -1, pct = -1, len_id = 0, len_name = -1;       // -1: the part is absent
    unsigned name[RL_MAX_CHARS / 4] = {};    // the bytes of the name's row, four to a word
    if (i < N) {
      // a block spends its time here waiting for loads, so they are issued together: first the label's own fields
      // (none depends on another), then -- they need the label -- its colour and the whole row of its name
      const long e = (long)b * N + i;
      const int label = labels[e];
      const float x1 = boxes[4 * e], y1 = boxes[4 * e + 1], x2 = boxes[4 * e + 2], y2 = boxes[4 * e + 3];
      if (idents) ident = idents[e];
      const float sc = scores ? scores[e] : __builtin_nanf("");
      if (label >= 0 && label < P && x1 == x1 && y1 == y1 && x2 == x2 && y2 == y2) {
        const unsigned char* c = palette + 3 * label;
        const unsigned red = c[0], green = c[1], blue = c[2];
        int n = 0, parts = 0;
        if (names && label < n_names) {
          const int first = label * name_stride, last = n_names * name_stride - 1;
          bool open = true;                  // no 0 so far
          len_name = 0;
#pragma unroll
          for (int j = 0; j < RL_MAX_CHARS; ++j) {             // no branch around a load: they all fly at once
            const unsigned byte = names[min(first + j, last)];                    // (past the row: bytes that are not used)
            name[j >> 2] |= byte << (8 * (j & 3));
            open = open && byte;
            len_name += open;
          }
          len_name = min(len_name, name_stride);
          n += len_name;
          ++parts;
        }
        if (ident >= 0) {
          len_id = 1;
          for (int v = ident; v >= 10; v /= 10) ++len_id;
          n += len_id;
          ++parts;
        }
        if (sc == sc) {
          pct = (int)fminf(fmaxf(sc * 100.f, 0.f), 99.f);
          n += 2;
          ++parts;
        }
        n = min(n + max(parts - 1, 0), RL_MAX_CHARS);
        if (n > 0) {
          const int Wp = (n * cw + 1) * s;
          const int lf = (int)fminf(fmaxf(x1, lo), hx), tp = (int)fminf(fmaxf(y1, lo), hy);
          int x0 = lf - t, y0 = tp - t - Hp;
          if (y0 < 0) y0 = tp;               // no room above the box: the caption moves inside
          x0 = max(min(x0, W - Wp), 0);
          y0 = max(min(y0, H - Hp), 0);
          r = make_int4(x0, y0, min(x0 + Wp, W), min(y0 + Hp, H));
          colour = red | (green << 8) | (blue << 16);
          if (299u * red + 587u * green + 114u * blue < 128000u) colour |= 1u << 24;
          keep = r.x < tx0 + RB_TILE_W && r.z > tx0 && r.y < ty0 + RB_TILE_H && r.w > ty0;
        }
      }
    }
    const unsigned long long votes = __ballot(keep);
    if (lane == 0) s_count[wave] = __popcll(votes);
    __syncthreads();
    int at = staged, total = 0;
#pragma unroll
    for (int w = 0; w < RB_WAVES; ++w) {
      if (w < wave) at += s_count[w];
      total += s_count[w];
    }
    if (keep) {
      at += __popcll(votes & ((1ull << lane) - 1ull));
      s_rect[at] = r;
      s_colour[at] = colour;
      // the characters: the parts that are present, one space between them, cut at RL_MAX_CHARS
      unsigned char* text = s_text + at * RL_MAX_CHARS;
      int pos = 0;
      bool sep = false;                      // a part came before: a space goes in front of the next one
      if (ident >= 0) {
        int v = ident;
        for (int j = len_id - 1; j >= 0; --j, v /= 10) text[j] = (unsigned char)('0' + v % 10);   // len_id <= 10
        pos = len_id;
        sep = true;
      }
      if (len_name >= 0) {
        if (sep) text[pos++] = ' ';          // pos <= 10 here
#pragma unroll
        for (int j = 0; j < RL_MAX_CHARS; ++j)
          if (j < len_name && pos + j < RL_MAX_CHARS) text[pos + j] = (unsigned char)(name[j >> 2] >> (8 * (j & 3)));
        pos += len_name;
        sep = true;
      }
      if (pct >= 0) {
        if (sep && pos < RL_MAX_CHARS) text[pos] = ' ';
        pos += sep;
        if (pos < RL_MAX_CHARS) text[pos] = (unsigned char)('0' + pct / 10);
        if (pos + 1 < RL_MAX_CHARS) text[pos + 1] = (unsigned char)('0' + pct % 10);
      }
    }
    staged += total;
    __syncthreads();                         // the counts are rewritten next round; after the last, the stage is whole
  }

  // ---- the plates
  const int x = tx0 + 4 * lane;
  if (x >= W) return;                        // (after the last barrier)
  for (int y = ty0 + wave; y < min(ty0 + RB_TILE_H, H); y += RB_WAVES) {
    const bool whole = x + 3 < W;
    const unsigned past = whole ? 0u : (0xFu << (W - x)) & 0xFu;   // bit j: pixel x + j lies past the row
    unsigned px[4] = {0u, 0u, 0u, 0u};
    unsigned done = past;                    // bit j: pixel x + j has met its topmost plate (or lies past the row)
    for (int k = staged - 1; k >= 0; --k) {
      if (__ballot(done != 0xFu) == 0) break;
      const int4 r = s_rect[k];
      const int x0 = uniform(r.x), y0 = uniform(r.y), x1 = uniform(r.z), y1 = uniform(r.w);
      if (y < y0 || y >= y1) continue;
      const unsigned hit = columns(x, x0, x1);
      const unsigned fresh = hit & ~done;
      if (fresh) {
        const unsigned info = (unsigned)uniform((int)s_colour[k]);
        const unsigned plate = info & 0xFFFFFFu, ink = (info >> 24 & 1u) ? 0xFFFFFFu : 0u;
        const int v = (int)((unsigned)(y - y0) * by_s >> 16) - 1;                 // the glyph row: the same in every lane
        const bool rows = v >= 0 && v < FH;
        const unsigned char* text = s_text + k * RL_MAX_CHARS;
        const unsigned char* glyph_row = s_font + (rows ? v : 0);
        // no branch per pixel, so that the LDS reads of the four overlap: a pixel outside the plate works on clamped
        // numbers and its result is dropped
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned a = (unsigned)min(max(x + j - x0, 0), 4095);
          const int u = (int)(a * by_s >> 16) - 1;                                // a / s - 1
          const unsigned uu = (unsigned)max(u, 0);
          const unsigned ci = min(uu * by_cw >> 16, (unsigned)RL_MAX_CHARS - 1u); // uu / cw; below n inside the plate
          const unsigned col = (uu - ci * (unsigned)cw) & 7u;
          const int g = (int)text[ci] - font_first;
          const bool has = g >= 0 && g < G;
          const unsigned bits = glyph_row[(has ? g : 0) * FH];
          const bool on = rows && u >= 0 && has && uu - ci * (unsigned)cw < (unsigned)FW && (bits >> (7u - col) & 1u);
          px[j] = (fresh >> j & 1u) ? (on ? ink : plate) : px[j];
        }
      }
      done |= hit;
    }
    const unsigned painted = done & ~past;
    if (!painted) continue;
    unsigned char* o = dst + (((long)b * H + y) * W + x) * 3;
    if (painted == 0xFu && ((uintptr_t)o & 3u) == 0) {
      unsigned* o4 = reinterpret_cast<unsigned*>(o);           // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
      o4[0] = px[0] | (px[1] << 24);
      o4[1] = (px[1] >> 8) | (px[2] << 16);
      o4[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (painted >> j & 1u) {
          o[3 * j] = (unsigned char)px[j];
          o[3 * j + 1] = (unsigned char)(px[j] >> 8);
          o[3 * j + 2] = (unsigned char)(px[j] >> 16);
        }
    }
  }
}

}  // namespace

extern "C" int fod_render_labels(unsigned char* pictures, int B, int H, int W, const float* boxes, const int* labels,
                                 int N, const int* idents, const float* scores, const unsigned char* names, int n_names,
                                 int name_stride, const unsigned char* palette, int P, const unsigned char* font,
                                 int font_first, int G, int FW, int FH, int scale, int thickness, hipStream_t stream) {
  FOD_REQUIRE(thickness >= 1, "render_labels: thickness %d is below 1", thickness);
  FOD_REQUIRE(N >= 0 && N <= RB_MAX_BOXES, "render_labels: %d labels per sample, not 0..%d", N, RB_MAX_BOXES);
  FOD_REQUIRE(P >= 1, "render_labels: a palette of %d colours", P);
  FOD_REQUIRE(H > 0 && W > 0 && (long)H >= 2L * thickness && (long)W >= 2L * thickness,
              "render_labels: a %dx%d picture does not hold bars of thickness %d", H, W, thickness);
  FOD_REQUIRE((long)3 * H * W <= INT_MAX, "render_labels: picture %dx%d is too large", H, W);
  FOD_REQUIRE(B > 0 && B <= 65535, "render_labels: %d pictures, not 1..65535", B);
  FOD_REQUIRE(scale >= 1 && scale <= 8, "render_labels: scale %d, not 1..8", scale);
  FOD_REQUIRE(FW >= 1 && FW <= 8 && FH >= 1 && FH <= 16, "render_labels: a %dx%d font cell, not 1..8 x 1..16", FW, FH);
  FOD_REQUIRE(font_first >= 0 && G >= 1 && font_first + (long)G <= 256,
              "render_labels: %d glyphs from code %d on do not lie in 0..255", G, font_first);
  FOD_REQUIRE(!names || (n_names >= 1 && n_names <= INT_MAX / RL_MAX_CHARS && name_stride >= 1 && name_stride <= RL_MAX_CHARS),
              "render_labels: a name table of %d rows of %d bytes (rows >= 1, bytes 1..%d)", n_names, name_stride,
              RL_MAX_CHARS);
  FOD_REQUIRE(pictures && font && (N == 0 || (boxes && labels && palette)), "render_labels: null pointer");
  const dim3 grid((W + RB_TILE_W - 1) / RB_TILE_W, (H + RB_TILE_H - 1) / RB_TILE_H, B);
  FOD_REQUIRE(grid.y <= 65535, "render_labels: picture %dx%d is too tall", H, W);
  if (N == 0 || !(idents || scores || names)) return FOD_OK;   // every text is empty: nothing is drawn
  hipLaunchKernelGGL(render_labels_kernel, grid, dim3(RB_THREADS), 0, stream, pictures, H, W, boxes, labels, N, idents,
                     scores, names, n_names, name_stride, palette, P, font, font_first, G, FW, FH, scale, thickness);
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}

extern "C" int fod_render_boxes(const void* src, int src_is_u8, unsigned char* dst, int B, int L, int H, int W,
                                long src_stride_b, long src_stride_l, const int* frame_idx, const float* mean,
                                const float* stdv, const float* boxes, const int* labels, int N,
                                const unsigned char* palette, int P, int thickness, hipStream_t stream) {
  FOD_REQUIRE(thickness >= 1, "render_boxes: thickness %d is below 1", thickness);
  FOD_REQUIRE(N >= 0 && N <= RB_MAX_BOXES, "render_boxes: %d boxes per sample, not 0..%d", N, RB_MAX_BOXES);
  FOD_REQUIRE(P >= 1, "render_boxes: a palette of %d colours", P);
  FOD_REQUIRE(H > 0 && W > 0 && (long)H >= 2L * thickness && (long)W >= 2L * thickness,
              "render_boxes: a %dx%d frame does not hold bars of thickness %d", H, W, thickness);
  FOD_REQUIRE((long)3 * H * W <= INT_MAX, "render_boxes: frame %dx%d is too large", H, W);
  FOD_REQUIRE(B > 0 && B <= 65535 && L > 0, "render_boxes: bad clip extent %dx%d", B, L);
  FOD_REQUIRE(src_stride_l >= (long)3 * H * W && src_stride_b >= (long)3 * H * W,
              "render_boxes: frame strides %ld / %ld overlap the 3x%dx%d planes", src_stride_b, src_stride_l, H, W);
  FOD_REQUIRE(src_is_u8 || (mean && stdv), "render_boxes: an f32 source needs mean and std (null pointer)");
  FOD_REQUIRE(src && dst && (N == 0 || (boxes && labels && palette)), "render_boxes: null pointer");
  const dim3 grid((W + RB_TILE_W - 1) / RB_TILE_W, (H + RB_TILE_H - 1) / RB_TILE_H, B);
  FOD_REQUIRE(grid.y <= 65535, "render_boxes: frame %dx%d is too tall", H, W);
  if (src_is_u8)
    hipLaunchKernelGGL(render_boxes_kernel<unsigned char>, grid, dim3(RB_THREADS), 0, stream,
                       (const unsigned char*)src, dst, L, H, W, src_stride_b, src_stride_l, frame_idx, mean, stdv, boxes,
                       labels, N, palette, P, thickness);
  else
    hipLaunchKernelGGL(render_boxes_kernel<float>, grid, dim3(RB_THREADS), 0, stream, (const float*)src, dst, L, H, W,
                       src_stride_b, src_stride_l, frame_idx, mean, stdv, boxes, labels, N, palette, P, thickness);
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}

extern "C" int fod_render_attention(const void* src, int src_is_u8, unsigned char* dst, int B, int L, int J, int H, int W,
                                    long src_stride_b, long src_stride_l, const int* frame_idx, const float* mean,
                                    const float* stdv, const float* maps, int h, int w, long map_stride_b,
                                    long map_stride_j, const float* colour_scale, const unsigned char* lut, float gain,
                                    float max_alpha, hipStream_t stream) {
  FOD_REQUIRE(src && dst && frame_idx && maps && colour_scale && lut, "render_attention: null pointer");
  FOD_REQUIRE(src_is_u8 || (mean && stdv), "render_attention: an f32 source needs mean and std (null pointer)");
  FOD_REQUIRE(h >= 1 && w >= 1 && (long)h * w <= INT_MAX, "render_attention: a %dx%d map", h, w);
  FOD_REQUIRE(J >= 1 && J <= 32, "render_attention: %d pictures per sample, not 1..32", J);
  FOD_REQUIRE(max_alpha >= 0.f && max_alpha <= 1.f, "render_attention: max_alpha %f outside [0, 1]", max_alpha);
  FOD_REQUIRE(fabsf(gain) <= 3.402823466e38f, "render_attention: gain is not finite");
  FOD_REQUIRE(H > 0 && W > 0 && (long)3 * H * W <= INT_MAX, "render_attention: bad frame %dx%d", H, W);
  FOD_REQUIRE(B > 0 && (long)B * J <= 65535 && L > 0, "render_attention: bad clip extent %dx%d", B, L);
  FOD_REQUIRE(src_stride_l >= (long)3 * H * W && src_stride_b >= (long)3 * H * W,
              "render_attention: frame strides %ld / %ld overlap the 3x%dx%d planes", src_stride_b, src_stride_l, H, W);
  FOD_REQUIRE(map_stride_b >= 0 && map_stride_j >= 0, "render_attention: negative map stride");
  const dim3 grid((W + RB_TILE_W - 1) / RB_TILE_W, (H + RB_TILE_H - 1) / RB_TILE_H, B * J);
  FOD_REQUIRE(grid.y <= 65535, "render_attention: frame %dx%d is too tall", H, W);
  if (src_is_u8)
    hipLaunchKernelGGL(render_attention_kernel<unsigned char>, grid, dim3(RB_THREADS), 0, stream,
                       (const unsigned char*)src, dst, L, J, H, W, src_stride_b, src_stride_l, frame_idx, mean, stdv, maps,
                       h, w, map_stride_b, map_stride_j, colour_scale, lut, gain, max_alpha);
  else
    hipLaunchKernelGGL(render_attention_kernel<float>, grid, dim3(RB_THREADS), 0, stream, (const float*)src, dst, L, J, H,
                       W, src_stride_b, src_stride_l, frame_idx, mean, stdv, maps, h, w, map_stride_b, map_stride_j,
                       colour_scale, lut, gain, max_alpha);
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}
