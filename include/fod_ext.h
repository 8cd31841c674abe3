/* fod_ext.h -- entry points of libfod_hip.so that came after include/fod.h was closed.
 *
 * Why a second header: fod.h is pinned as a whole -- its prototypes, structs and served entry points are counted by
 * the tests that keep the binding (future_od/native/abi.py, lib.py) and the fast-call wrappers equal to it, and those
 * counts are a yardstick that later work does not move.  An entry point that is added without changing anything fod.h
 * declares goes here instead.  Same dialect, same conventions (fod.h's opening comment: device pointers, asynchronous on
 * `stream`, nothing allocated, no state kept, 0 on success and the text via fod_last_error()), read by the same reader:
 * abi.py hands it fod.h's pointer typedefs and keeps its prototypes in tables of their own (EXT_PROTOTYPES), lib.py
 * types and binds them so that lib.call(name, ...) serves them.  This header declares prototypes only: no struct, no
 * constant, no name fod.h has.  FOD_ABI_VERSION (fod.h) counts for both.
 */
#ifndef FOD_EXT_H_
#define FOD_EXT_H_

#include "fod.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Exponential moving average of the weights over many tensors in ONE launch (the reference has none; what a
 * DETR-family trainer keeps beside its optimizer, torch: `ema.lerp_(p, 1 - d)` per tensor).  Device tables with the
 * geometry of fod_multi_adamw:
 *   pairs i64 [T,2] = {average, parameter} f32 pointers (same dense layout each), numel i64 [T]; block b works on
 *   elements [blk_chunk[b]*C, +C) of pair blk_tensor[b], C = fod_multi_chunk().
 * updates_dev: i64 device scalar, the number u >= 1 of THIS update -- advanced on the stream by the caller before the
 * launch, so a captured launch bakes in no count.  Every block forms the weight itself, in double:
 *   d = warmup ? min((double)decay, (1 + u) / (10 + u)) : (double)decay,   w = (float)(1 - d)
 * and every element becomes  e = e + w * (p - e)  with the subtraction, the product and the sum each rounded to f32
 * (no fused multiply-add): a float32 restatement gives the same bits.  Reads p and e, writes e (12 B / element).
 * 16-byte accesses where both tensors of a pair are 16-byte aligned, a scalar tail; 4-byte accesses otherwise.
 * decay outside [0, 1] is FOD_ERR_ARG. */
int fod_multi_ema(const long* pairs, const long* numel, const int* blk_tensor, const int* blk_chunk, int nblocks,
                  const long long* updates_dev, float decay, int warmup, fod_stream_t stream);
/* The two tensors of every pair exchange their contents, bit for bit (words are moved, not interpreted); twice is the
 * identity.  Same tables as fod_multi_ema.  The tensors of a pair must not overlap. */
int fod_multi_swap(const long* pairs, const long* numel, const int* blk_tensor, const int* blk_chunk, int nblocks,
                   fod_stream_t stream);
/* Gradient accumulation over many tensors in ONE launch: what a trainer does between the backward passes of the
 * micro-batches of one update (torch: `acc.add_(g)` per tensor, then `g.div_(n)`).  Same tables as fod_multi_ema, with
 *   pairs i64 [T,2] = {accumulator, gradient} f32 pointers (same dense layout each, not overlapping).
 * mode (a number: this header declares no constants):
 *   0  store   acc = g                   words are moved, not interpreted; g is untouched           (8 B / element)
 *   1  add     acc = acc + g             g is untouched                                             (12 B / element)
 *   2  finish  g = (acc + g) * scale     acc is untouched; the sum and the product are each rounded to f32
 *                                        (no fused multiply-add)                                    (12 B / element)
 * so N micro-batches -- store, N - 2 adds, finish with scale = (float)(1.0 / N) -- leave
 *   (((g1 + g2) + g3) + ... + gN) * scale  in the gradient tensors, where the optimizer reads it; a float32 restatement
 * gives the same bits.  No atomics, every element is written by exactly one thread: the result does not depend on timing.
 * scale is read by mode 2 only and checked in every mode.  16-byte accesses where both tensors of a pair are 16-byte
 * aligned, a scalar tail; 4-byte accesses otherwise.  A mode outside 0..2, or a scale that is not finite or not > 0, is
 * FOD_ERR_ARG. */
int fod_multi_accum(const long* pairs, const long* numel, const int* blk_tensor, const int* blk_chunk, int nblocks,
                    int mode, float scale, fod_stream_t stream);
/* fod_clip_crop_resize (fod.h) with the photometric half of the augmentation in the same pass: brightness, contrast,
 * saturation and hue jitter, drawn once per clip and applied identically to its L frames.  Arguments, geometry and
 * checks are fod_clip_crop_resize's, plus
 *   photo: DEVICE f32 [B][5] = (delta, alpha, sat, hue, first), one row per clip: brightness added on the 0..1 scale,
 *   contrast factor, saturation factor, hue rotation in turns, and first != 0: contrast before the HSV stage, else after.
 * The map mixes the three planes of a pixel: C must be 3 (anything else is FOD_ERR_ARG).  The neutral row is
 * (0, 1, 1, 0, any).  For a pixel p = (r, g, b) = the bilinear sample / 255 (what fod_clip_crop_resize holds just before
 * it normalises), every step in f32:
 *   1. p += delta
 *   2. if first: p *= alpha
 *   3. only if sat != 1 or hue != 0, the HSV stage:
 *        p = clamp(p, 0, 1);  v = max(r, g, b), m = min(r, g, b), c = v - m;  s = c > 0 ? c / v : 0
 *        h6 = 0 if c == 0;  else fmod((g - b) / c, 6) made non-negative if v == r;  else (b - r) / c + 2 if v == g;
 *             else (r - g) / c + 4;   h = h6 / 6
 *        s = min(s * sat, 1);  h = h + hue, h -= floor(h)
 *        with k(n) = fmod(n + 6 h, 6) and f(n) = v - v * s * max(0, min(k, 4 - k, 1)):  (r, g, b) = (f(5), f(3), f(1))
 *   4. if not first: p *= alpha
 *   5. p = clamp(p, 0, 1)
 *   6. (p[c] - mean[c]) / std[c], as fod_clip_crop_resize
 * The map is continuous in (r, g, b): a grey pixel has s = 0, so its undefined hue never reaches the output.  A clip
 * whose row is neutral skips steps 1-5: its output is bit-equal to fod_clip_crop_resize's.
 * The row is read by the kernel and never trusted: a non-finite delta, alpha, sat or hue is replaced by its neutral
 * value; then delta is clamped to [-1, 1], alpha and sat to [0, 4], and hue becomes hue - floor(hue); first counts as set
 * unless it equals 0.  Whatever the row holds, every output is finite. */
int fod_clip_crop_resize_photo(const unsigned char* src, float* dst, int B, int L, int C, int H0, int W0, int H, int W,
                               long src_stride_b, long src_stride_l, const int* plans, const float* mean,
                               const float* std, const float* photo, fod_stream_t stream);
/* fod_clip_crop_resize with ANTIALIASED resampling: where the crop rectangle is larger than the output, every output
 * value averages the whole source footprint under a triangle filter instead of sampling two taps per axis (which at a
 * ratio of 2 never reads half of the source).  The definition is
 *   torch.nn.functional.interpolate(crop, size=(H, W), mode="bilinear", align_corners=False, antialias=True)
 * on the (clamped) crop rectangle of the raw 0..255 values, then the pixel pipeline of fod_clip_crop_resize.  Per axis,
 * with n_in the rectangle's extent and n_out the output's:
 *   scale = n_in / n_out,   sup = max(scale, 1)
 *   for output index i:   c = scale * (i + 0.5),   lo = max(0, int(c - sup + 0.5)),   hi = min(n_in, int(c + sup + 0.5))
 *   w_j = max(0, 1 - |(j - c + 0.5) / sup|)  for j in [lo, hi),  each divided by their sum
 * (int() truncates towards zero).  The horizontal pass runs first, the vertical pass second, both in f32 on the 0..255
 * values; then ((v / 255) - mean[c]) / std[c].  Taps are clamped to the crop rectangle, never to the frame: no pixel
 * outside the rectangle reaches the output.  flip mirrors the output columns.  A rectangle of the output's size comes
 * out bit-equal to fod_clip_crop_resize (the weights are 1 and 0); an enlarged axis has the weights of plain bilinear.
 * (The kernel forms x / sup and w / sum as products with one reciprocal per axis and output: within an ulp of the
 * quotient, exact where sup or the sum is 1.)
 * Arguments, the plan rows (read from device memory and clamped into the frame), the checks and the 16-byte alignment
 * are fod_clip_crop_resize's, plus
 *   photo: NULL, or DEVICE f32 [B][5] as fod_clip_crop_resize_photo takes it: steps 1-5 of that map are then applied to
 *   the antialiased sample / 255 before it is normalised (C must then be 3; anything else is FOD_ERR_ARG).  The row is
 *   sanitised as there; a neutral row gives the bits of a NULL photo.
 * The footprint follows the clamped rectangle, per clip and per axis, at run time.  What is accepted is decided from
 * (H0, W0, H, W) alone, before any launch and never from plan contents: H0 <= 4 * H and W0 <= 4 * W (a rectangle lies
 * inside its frame, so no axis is reduced by more than 4); a larger frame is FOD_ERR_ARG and nothing is written.
 * Not this: torchvision's uint8 path with integer weights (this is the float path's definition), bicubic. */
int fod_clip_crop_resize_aa(const unsigned char* src, float* dst, int B, int L, int C, int H0, int W0, int H, int W,
                            long src_stride_b, long src_stride_l, const int* plans, const float* mean,
                            const float* std, const float* photo, fod_stream_t stream);
/* Visualisation: one frame of each sample of a clip as an 8-bit RGB picture with box outlines painted on it, in ONE
 * launch (the reference's revert_imagenet_normalization + draw_boxes + `* 255` + `.byte()`, which it runs on the host
 * after copying the whole f32 clip there).  future_od/utils/visualization.py (draw_boxes, render) is the CPU form.
 *   src: [B][L][3][H][W], planar and dense inside a frame, src_stride_b / src_stride_l in ELEMENTS (each at least
 *        3*H*W); src_is_u8 == 0: f32, normalised with mean / std (DEVICE f32 [3] each); != 0: raw uint8 (mean / std are
 *        not read and may be NULL).
 *   frame_idx: DEVICE i32 [B], the frame of each sample, or NULL for frame 0.  A negative value counts from the end
 *        (-1 is L - 1); after that step the value is clamped into [0, L).
 *   dst: uint8 [B][H][W][3], interleaved RGB (a PNG scanline).
 * Background pixel, per channel c.  f32:  v = x * std[c] + mean[c],  w = v * 255 -- the product, the sum and the second
 * product each rounded to f32, no fused multiply-add, as in fod_multi_ema -- then w truncated towards zero and clamped
 * to 0..255; a w that is not finite (NaN, +-inf) gives 0.  uint8: the byte is copied.  (The reference's `.byte()` of an
 * out-of-range float is undefined; this clamps.)
 * Boxes: boxes f32 [B][N][4], xyxy in pixels of the frame; labels i32 [B][N]; palette DEVICE uint8 [P][3].  Box n of a
 * sample is DRAWN iff 0 <= label < P and none of its four coordinates is NaN; its colour is palette[label].  With
 * t = thickness, all in f32 and then truncated to int:
 *   Lf = trunc(min(max(x1, t), W - t))   Rt = trunc(min(max(x2, t), W - t))
 *   Tp = trunc(min(max(y1, t), H - t))   Bt = trunc(min(max(y2, t), H - t))
 * and pixel (y, x) lies on the box's outline iff it lies in one of four bars:
 *   left:    Tp - t <= y < Bt       and  Lf - t <= x < Lf
 *   bottom:  Bt     <= y < Bt + t   and  Lf - t <= x < Rt
 *   right:   Tp     <= y < Bt + t   and  Rt     <= x < Rt + t
 *   top:     Tp - t <= y < Tp       and  Lf     <= x < Rt + t
 * An empty range holds nothing: a reversed or collapsed box draws the bars that remain (what slicing does in the
 * reference); the clamps keep every bar inside the picture; +-inf clamps like any other value.  A pixel takes the colour
 * of the HIGHEST-index drawn box whose outline holds it (the painter's order: later boxes cover earlier ones), else its
 * background.  N == 0 converts only (boxes, labels and palette may then be NULL).
 * FOD_ERR_ARG before any launch: thickness < 1; H or W below 2 * thickness; N < 0 or N > 1024 (the matcher's query
 * limit); P < 1; an f32 source without mean or std; a NULL src or dst; strides below 3*H*W; B outside 1..65535.
 * Reads 12 B (f32) or 3 B (uint8) and writes 3 B per pixel; 16-byte loads and dword stores where a row's addresses
 * allow, element by element otherwise (no alignment is required of any pointer). */
int fod_render_boxes(const void* src, int src_is_u8, unsigned char* dst, int B, int L, int H, int W, long src_stride_b,
                     long src_stride_l, const int* frame_idx, const float* mean, const float* std, const float* boxes,
                     const int* labels, int N, const unsigned char* palette, int P, int thickness, fod_stream_t stream);
/* Attention maps for looking at a trained model: the head-averaged cross-attention of SELECTED queries over the keys of
 * up to 32 memory images in ONE launch (the reference's demo.ipynb reads SlotToImageAttention.stored_attention, the head
 * mean of the softmax weights, one block at a time).
 *   ptrs: HOST array of njobs x 4 addresses in the order q1, q2, k1, k2 (q2 / k2 NULL for all jobs or for none), 16-byte
 *        aligned; njobs is 1..32.  The addresses travel in the kernel arguments, as in fod_attn_bwd_dkv_multi: a captured
 *        launch needs no table in memory.  A job is one memory image: its queries [B,Tq,H*32], its keys [B,S,H*32].
 *   shape: B, H (at most 64), Tq, S, the q / k / k2 strides and scale are honoured exactly as fod_attn_fwd honours them
 *        (k2_token_stride = 0: the strides of k1; k2_batch_stride = 0: one positional key table shared by the batch;
 *        strides are multiples of 8 elements).  The v / o strides, the split scratch and dq_scale are not read.
 *        drop_p != 0 is FOD_ERR_ARG: the map is the probabilities before dropout.
 *   query_idx: DEVICE i32 [B][Q], or NULL for the identity with Q == Tq.  An index outside [0, Tq) gives a row of zeros
 *        (the padding of fod_detect_select is -1); duplicates are allowed.
 *   out: f32 [B][Q][njobs][S], dense:
 *        out[b,i,j,s] = (1/H) sum_h softmax_s((q1_h . k1_h + q2_h . k2_h) * scale)   for query query_idx[b,i] of job j,
 *        head h = channels [32h, 32h+32).  Every element is written, by exactly one thread; no atomics: the result does
 *        not depend on timing.
 * dtype FOD_BF16: the products are exact and summed in f32; FOD_F32: an f32 fma chain on the unrounded operands.  With
 * x = score * (scale * log2 e) rounded to f32, an element is 2^((x - max2) - log2 sum2) with max2 the row maximum of x
 * and sum2 the f32 sum of 2^(x - max2) over the row, each 2^ one v_exp_f32; the head mean is the f32 sum times (1/H).
 * FOD_ERR_ARG before any launch: njobs outside 1..32; Q or Tq outside 1..1024; S < 1; q2 / k2 given for some jobs or
 * operands only; a NULL out, ptrs, shape, q1 or k1; NULL query_idx with Q != Tq; drop_p != 0; H above 64; a misaligned
 * operand or stride. */
int fod_attn_maps(int dtype, int njobs, const void* const* ptrs, const int* query_idx, int Q, float* out,
                  const fod_attn_shape* shape, fod_stream_t stream);
/* Visualisation: the maps of one detection per sample blended over their past frames, B x J pictures in ONE launch (the
 * reference's demo.ipynb upsamples every query's map with F.interpolate and blends with matplotlib on the host).
 * future_od/utils/visualization.py (render_attention) is the CPU form.  Picture (b, j) is frame frame_idx[b][j] of the
 * clip with map (b, j) over it.
 *   src, src_is_u8, L, H, W, src_stride_b, src_stride_l, mean, std: as fod_render_boxes, and so is the background BYTE
 *        bg of a pixel and channel (f32: (x * std + mean) * 255 in three roundings, truncated, clamped, not finite -> 0).
 *   frame_idx: DEVICE i32 [B][J]; a negative value counts from the end, then the value is clamped into [0, L).
 *   maps: f32 [h][w] per (b, j) at maps + b * map_stride_b + j * map_stride_j (ELEMENTS; rows dense).
 *   colour_scale: DEVICE f32 [B][J];  lut: DEVICE uint8 [256][3];  dst: uint8 [B][J][H][W][3], interleaved RGB.
 * Per pixel (y, x), every step ONE f32 operation, no fused multiply-add:
 *   fy = max(((y + 0.5) * (h / H)) - 0.5, 0)   (F.interpolate's bilinear coordinate, align_corners=False; h / H is one
 *   f32 division), y0 = min(trunc(fy), h - 1), y1 = min(y0 + 1, h - 1), wy1 = fy - y0, wy0 = 1 - wy1; likewise x.
 *   top = m[y0][x0] * wx0 + m[y0][x1] * wx1,  bot = m[y1][x0] * wx0 + m[y1][x1] * wx1,  a = top * wy0 + bot * wy1
 *   alpha = min(max(a * gain, 0), max_alpha)
 *   colour = lut[trunc(min(max(a * colour_scale[b][j], 0), 1) * 255)]
 *   byte[c] = trunc(min(max(bg[c] * (1 - alpha) + colour[c] * alpha, 0), 255))
 * where max(v, 0) of a NaN v is 0.  An a that is not finite (NaN, +-inf) leaves the background byte.  gain = 0 or
 * max_alpha = 0 gives fod_render_boxes' picture without boxes.  The reference's values are gain 50, max_alpha 0.4.
 * FOD_ERR_ARG before any launch: a NULL src, dst, frame_idx, maps, colour_scale or lut; an f32 source without mean or
 * std; h or w below 1; J outside 1..32; max_alpha outside [0, 1]; a gain that is not finite; strides below 3*H*W; a
 * negative map stride; B * J above 65535. */
int fod_render_attention(const void* src, int src_is_u8, unsigned char* dst, int B, int L, int J, int H, int W,
                         long src_stride_b, long src_stride_l, const int* frame_idx, const float* mean, const float* std,
                         const float* maps, int h, int w, long map_stride_b, long map_stride_j,
                         const float* colour_scale, const unsigned char* lut, float gain, float max_alpha,
                         fod_stream_t stream);
/* Visualisation: captions -- index, class name and score of every drawn box as text on a plate above it -- painted IN
 * PLACE on the uint8 [B][H][W][3] pictures fod_render_boxes wrote, in ONE launch (the reference's notebook writes every
 * detection's index with cv2.putText on the host; its W&B boxes carry "<idx> <category>" and a score).  The text is
 * composed and rasterised by the kernel: nothing is read back.  future_od/utils/visualization.py (label_text,
 * draw_labels) is the CPU form.  Integer arithmetic throughout, except the one f32 product of the score.
 *   boxes f32 [B][N][4], labels i32 [B][N], palette DEVICE uint8 [P][3], thickness: as handed to fod_render_boxes.
 *        Label n of sample b is DRAWN iff box n is: 0 <= label < P and no coordinate is NaN.  Lf and Tp are that
 *        function's integers (clamped to [t, W - t] / [t, H - t] in f32, then truncated; t = thickness).
 *   idents i32 [B][N], scores f32 [B][N], names uint8 [n_names][name_stride] (name_stride <= 32): each may be NULL.
 *   font: DEVICE uint8 [G][FH], one byte per glyph row; the glyph of character code c is row c - font_first, column
 *        col of a row is bit 7 - col (the most significant bit is leftmost); 1 <= FW <= 8, 1 <= FH <= 16.  A code
 *        outside [font_first, font_first + G) draws as a blank cell.
 * Text: at most FOD_LABEL_MAX_CHARS = 32 bytes (a number: this header declares no constants) -- the parts that are
 * PRESENT, joined by one space (0x20), then cut at 32:
 *   the decimal digits of ident (no sign, no padding), present iff idents is given and ident >= 0;
 *   the bytes of names[label] up to its first 0 (a row without a 0 is name_stride bytes long), present iff names is
 *        given and label < n_names -- present also when it is empty, so its space is kept;
 *   two decimal digits of pct = min(99, max(0, trunc(score * 100.f))), present iff scores is given and the score is not
 *        NaN; the product is one f32 multiplication, +inf gives 99, 0.07 gives "07".
 * An empty text draws nothing.  Geometry, with s = scale, n = the number of characters:
 *   Wp = (n * (FW + 1) + 1) * s,  Hp = (FH + 2) * s
 *   x0 = Lf - t,  y0 = Tp - t - Hp;  if y0 < 0 then y0 = Tp (the caption moves inside the box)
 *   x0 = max(min(x0, W - Wp), 0),  y0 = max(min(y0, H - Hp), 0)
 * The plate is rows [y0, y0 + Hp) x columns [x0, x0 + Wp), clipped to the picture.  For a plate pixel (x, y):
 *   u = (x - x0) / s - 1,  v = (y - y0) / s - 1   (integer division of non-negative numbers)
 * and the pixel is INK iff u >= 0, 0 <= v < FH, u % (FW + 1) < FW, and bit 7 - u % (FW + 1) of row v of the glyph of
 * character u / (FW + 1) is set; any other plate pixel takes the plate colour.  The plate is opaque in palette[label];
 * with lum = 299 R + 587 G + 114 B of it the ink is black (0, 0, 0) if lum >= 128000 and white (255, 255, 255) otherwise.
 * Painter's order: among the plates that cover a pixel the HIGHEST n wins, plate and ink together.  Pixels outside
 * every plate are neither read nor written, so all captions lie above all outlines; every written byte has exactly one
 * writer, no atomics.  N == 0, or idents, scores and names all NULL, draws nothing (no launch).
 * FOD_ERR_ARG before any launch: thickness < 1; H or W below 2 * thickness; N < 0 or N > 1024; P < 1; scale outside
 * 1..8; FW outside 1..8; FH outside 1..16; font_first < 0, G < 1 or font_first + G > 256 (codes are bytes); names with
 * n_names < 1 (or above INT_MAX / 32) or name_stride outside 1..32; a NULL pictures or font; NULL boxes, labels or palette with N > 0; B outside
 * 1..65535.
 * Every block reads each label (up to 28 B and its name) and writes 3 B per plate pixel of its tile; dword stores where
 * four consecutive pixels of a row are all painted and their address allows, byte stores otherwise (no alignment is
 * required of any pointer). */
int fod_render_labels(unsigned char* pictures, int B, int H, int W, const float* boxes, const int* labels, int N,
                      const int* idents, const float* scores, const unsigned char* names, int n_names, int name_stride,
                      const unsigned char* palette, int P, const unsigned char* font, int font_first, int G, int FW,
                      int FH, int scale, int thickness, fod_stream_t stream);
/* Duplicate suppression behind fod_detect_select: greedy hard NMS over the rows that function wrote, per sample, in ONE
 * launch (the reference has none; torchvision.ops.nms / batched_nms is the usual host-side form).  One workgroup per
 * sample, wave64, no scratch, no atomics, nothing between workgroups: two launches give equal bits, and the launch can
 * be captured.  ops.detect_nms on CPU tensors is the plain form of the same definition.
 *   scores f32 [B][K], labels i32 [B][K], boxes f32 [B][K][4] xyxy, query i32 [B][K], count i32 [B]: the five tensors
 *        of fod_detect_select, dense.  Nothing but 4-byte alignment is required of any pointer.
 * Candidates and order: rows j < n = min(max(count[b], 0), K) of sample b, in ROW order -- the order fod_detect_select
 * left them in: score descending, ties by flat index.  Scores are never read for ordering; rows at or beyond count[b]
 * are never read at all.  Row j is KEPT iff no kept row i < j suppresses it.
 * Row i SUPPRESSES row j iff
 *   (class_agnostic != 0  or  labels[i] == labels[j])   and   inter > iou_threshold * uni
 * with, all in f32, every operation rounded once, no fused multiply-add:
 *   w = max(x1 - x0, 0),  h = max(y1 - y0, 0),  area = w * h                       (inverted corners: area 0)
 *   iw = max(min(x1_i, x1_j) - max(x0_i, x0_j), 0),  ih likewise in y,  inter = iw * ih
 *   uni = (area_i + area_j) - inter
 * There is no division: iou_threshold = 0.5 on boxes with small-integer corners is decided exactly, an IoU EQUAL to the
 * threshold does not suppress, and two zero-area boxes never suppress each other (0 > 0 is false).
 * A row with a NaN or infinite coordinate is kept and suppresses nothing: this is tested explicitly, before any min /
 * max sees the value.
 * Output: the survivors at the front of out_scores / out_labels / out_boxes / out_query in their original order, each
 * row copied bit for bit; out_count[b] = their number; out_source i32 [B][K] (may be NULL) = the input row each output row
 * came from.  Rows from out_count[b] on are the padding of fod_detect_select: score 0, label -1, query -1, box 0, and
 * source -1.  Every one of the B * K output rows is written, by exactly one thread.
 * Every output may alias its input (in place): the workgroup holds all rows of its sample before it writes any.
 * class_agnostic = 0 compares labels; anything else compares boxes only.
 * FOD_ERR_ARG before any launch: K outside 1..1024 (the limit of fod_detect_select: every result of it is accepted);
 * B < 1; an iou_threshold that is not finite or outside [0, 1]; a NULL operand other than out_source.
 * Not this: soft-NMS, a division-based `inter / uni > thr` where the two round differently, suppression across samples. */
int fod_detect_nms(const float* scores, const int* labels, const float* boxes, const int* query, const int* count, int B,
                   int K, float iou_threshold, int class_agnostic, float* out_scores, int* out_labels, float* out_boxes,
                   int* out_query, int* out_count, int* out_source, fod_stream_t stream);

/* AP bookkeeping over DETECTION ROWS: fod_od_map's greedy true / false-positive assignment (fod.h; reference
 * utils/od_map.py:214-287), with the ranked candidates taken from the rows of fod_detect_select / fod_detect_nms instead
 * of from dense scores, so that top_k, score_threshold, per_query and the suppression show in the AP.  ONE launch, one
 * workgroup per (class, sample) with T waves of 64, one IoU threshold each; no scratch, no atomics, nothing between
 * workgroups: two launches give equal bits, and the launch can be captured.  ops.detect_od_map on CPU tensors is the
 * plain form of the same definition.
 *   scores f32 [B][K], labels i32 [B][K], boxes f32 [B][K][4] xyxy, query i32 [B][K], count i32 [B]: the five tensors of
 *        fod_detect_select / fod_detect_nms, dense.  Boxes in the frame of the annotations (no box_map).
 *   anno_boxes f32 [B][N][4] xyxy, anno_classes i64 [B][N], anno_active i64 [B][N]: the dense annotations of fod_od_map.
 *   C real classes, C1 = C + 1 (class C is the generic class); P candidate slots per sample and class; T thresholds.
 * Outputs, fod_od_map's layout with P in place of min(50, M):
 *   confs f32 [T][C1][B*P], is_positive u8 [T][C1][B*P], size_categories u8 [C1][4][B*P], num_annos i64 [C1][4].
 * Per sample b, n = min(max(count[b], 0), K); rows at or beyond n are never read.
 * Candidates of class c < C: the rows j < n with labels[j] == c, in row order.  Candidates of the generic class c == C:
 * the rows j < n for which no earlier row i < j has query[i] == query[j] (each query's best surviving row; with per_query
 * rows: every row).  In both cases only the first P candidates count, and ROW ORDER IS THE RANKING: scores are never
 * compared.
 * Slot b*P + k holds candidate k: confs = its score for every t; size flags as fod_od_map's: column 0 is 1, columns 1..3
 * are  area <= s0,  s0 < area <= s1,  s1 < area  with the UNCLAMPED area (x1 - x0) * (y1 - y0) and
 * s0 = (float)(1/24 * 1/64 * img_h * img_w), s1 = (float)(1/4 * 1/12 * img_h * img_w) formed in double.
 * Slots k >= the number of candidates are padding: confs 0, is_positive 0, all four flags 0 (they add to no cumulative
 * sum of the AP).
 * Assignment, for threshold t with thr = (float)(0.5 + t * 0.05) (fod_od_map's): walk the candidates in order; each
 * claims the still-free annotation of greatest IoU, ties to the lowest index; it is positive iff that IoU >= thr, and the
 * annotation is then taken.  Free at the start: active == 1, and for c < C also class == c.  The IoU is fod_od_map's,
 * in f32, every operation rounded once, no fused multiply-add:
 *   area = max(x1 - x0, 0) * max(y1 - y0, 0),  inter = max(min(x1, X1) - max(x0, X0), 0) * (likewise in y)
 *   iou = (inter + 1e-7f) / (((area_p + area_a) - inter) + 1e-7f)            (two zero-area boxes: IoU 1)
 * num_annos[c][s] = the annotations of all samples that are free at the start for c, by the same size flags; written by
 * this launch, it needs no zeroing.  Every element of every output is written exactly once.
 * Non-finite input, tested explicitly before any min / max: a row with a NaN or infinite coordinate keeps its slot and
 * its score, gets flags (1, 0, 0, 0), is never positive and claims nothing; an active annotation with such a coordinate
 * counts in column 0 of num_annos only and can never be claimed.
 * With every (query, class) pair selected (K = M * C, threshold 0) and P = min(50, M) the four outputs equal fod_od_map's
 * on the same predictions, element for element.
 * FOD_ERR_ARG before any launch: B < 1; K outside 1..1024; N outside 1..1024; P outside 1..K; T outside 1..16; C < 1;
 * a NULL operand.
 * Not this: COCO's 101-point interpolation, detections in another frame than the annotations, more than 1024 rows. */
int fod_detect_od_map(const float* scores, const int* labels, const float* boxes, const int* query, const int* count,
                      const float* anno_boxes, const int64_t* anno_classes, const int64_t* anno_active, float* confs,
                      uint8_t* is_positive, uint8_t* size_categories, int64_t* num_annos, int B, int K, int N, int C,
                      int P, int T, float img_h, float img_w, fod_stream_t stream);

/* Identities across calls: associate the detection rows of ONE call with the tracks the caller keeps from the calls
 * before it, age and retire the tracks nobody claimed, and start new ones -- per sample, in ONE launch (the reference
 * has none; fod_tracker_cost / fod_tracker_extrapolate are its prediction baseline, inside one forward, and keep no
 * state).  One workgroup per sample, wave64, no scratch, no atomics, nothing between workgroups: two launches from
 * equal states give equal bits, and the launch can be captured.  ops.track_update on CPU tensors is the plain form of
 * the same definition.
 *   scores f32 [B][K], labels i32 [B][K], boxes f32 [B][K][4] xyxy, count i32 [B]: read only, the dense tensors of
 *        fod_detect_select / fod_detect_nms (their `query` is not needed).
 *   Track state, S slots per sample, owned by the caller and updated IN PLACE:
 *        trk_boxes f32 [B][S][4] the last associated box; trk_vel f32 [B][S][4] the displacement of every corner per
 *        call; trk_meta i32 [B][S][4] = (id, label, hits, misses); trk_scores f32 [B][S]; next_id i32 [B].
 *        A slot is LIVE iff id >= 0.  The other fields of a free slot are never read, and never written unless a track
 *        is born there.  No state tensor may alias a detection tensor or an output.
 *   out_track i32 [B][K], out_hits i32 [B][K], out_slot i32 [B][K] (may be NULL).
 *   Nothing but 4-byte alignment is required of any pointer.
 * Per sample b, n = min(max(count[b], 0), K); rows at or beyond n are never read.  All arithmetic is f32, every
 * operation rounded once, no fused multiply-add.
 * 1. Prediction.  A live slot has gap = (float)(misses + 1) and the predicted box  box + vel * gap  per corner (one
 *    multiplication, one addition) if motion != 0, and  box  otherwise.  A live slot whose predicted box has a NaN or
 *    infinite corner cannot be claimed; it ages like any unclaimed slot (4).
 * 2. Claims -- fod_detect_od_map's procedure with tracks in place of annotations.  The rows j < n are walked in ROW
 *    order; scores are never compared.  A row with a NaN or infinite corner (tested explicitly, before any min / max
 *    sees the value) claims nothing and is never born.  Any other row looks at the live, claimable slots that no
 *    earlier row has claimed -- with class_agnostic == 0 only at those with label == labels[j] -- and CHOOSES the one of
 *    greatest IoU with the predicted box, ties to the lowest slot index (no such slot: no match).  With the row's box
 *    (x0, y0, x1, y1) and the predicted box (X0, Y0, X1, Y1):
 *      area = max(x1 - x0, 0) * max(y1 - y0, 0)                                       (inverted corners: area 0)
 *      inter = max(min(x1, X1) - max(x0, X0), 0) * max(min(y1, Y1) - max(y0, Y0), 0)
 *      uni = (area_row + area_slot) - inter,   iou = uni > 0 ? inter / uni : 0        (uni NaN: 0)
 *    One division, no smoothing term: zero-area boxes match nothing.  The row is MATCHED iff, for the CHOSEN slot,
 *    inter > 0 and iou >= iou_threshold; the slot is then claimed.  Otherwise it stays free for later rows.
 * 3. A slot s matched by row j:  vel = (row_box - box) / gap per corner (one subtraction, one division; 0 if
 *    motion == 0), then box = row_box, score = scores[j], label = labels[j], hits += 1, misses = 0;
 *    out_track[j] = id, out_hits[j] = the new hits, out_slot[j] = s.
 * 4. A live slot nobody claimed: misses += 1; if misses > max_misses the slot is cleared: meta (-1, -1, 0, 0), box,
 *    vel and score 0.
 * 5. Births.  The candidates are the unmatched rows j < n of finite corners with scores[j] >= birth_score (a NaN
 *    score never qualifies), in row order.  The r-th candidate (r = 0, 1, ...) takes the r-th free slot in ascending
 *    slot order, free as judged AFTER step 4: id = next_id[b] + r, the row's box, score and label, vel 0, hits 1,
 *    misses 0; out_track = that id, out_hits = 1, out_slot = the slot.  Candidates beyond the free slots stay
 *    untracked.  next_id[b] grows by the number born.
 * 6. Every other row, rows at or beyond n included: out_track -1, out_hits 0, out_slot -1.  Each of the B * K output
 *    rows has exactly one writer.
 * class_agnostic = 0 compares labels; anything else compares boxes only.
 * FOD_ERR_ARG before any launch: K or S outside 1..1024; B < 1; an iou_threshold that is not finite or outside [0, 1];
 * max_misses < 0; a NULL operand other than out_slot.
 * The launch reads 24 B per row below count and up to 52 B per slot, and writes 12 B per row and up to 52 B per slot.
 * Not this: Hungarian association, Kalman filters, appearance features, identities across samples, ids that wrap
 * beyond 2^31 - 1, more than 1024 rows or slots. */
int fod_track_update(const float* scores, const int* labels, const float* boxes, const int* count, int B, int K,
                     float* trk_boxes, float* trk_vel, int* trk_meta, float* trk_scores, int* next_id, int S,
                     float iou_threshold, float birth_score, int max_misses, int class_agnostic, int motion,
                     int* out_track, int* out_hits, int* out_slot, fod_stream_t stream);

/* Streaming AP: the four tensors of the AP bookkeeping (fod_od_map or fod_detect_od_map) are folded, batch after batch,
 * into INTEGER histograms over score bins; one finalising launch turns them into the reference's AP, COCO's 101-point
 * interpolated AP, a precision / recall curve and the operating point.  The state has a constant size, its sums are
 * exact and independent of order (two runs give equal bits although the adds are atomic), and several processes combine
 * theirs by adding the three tensors element-wise.  Both launches can be captured.  ops.ap_hist_accum / ap_hist_finalize
 * on CPU tensors are the plain form of the same definition.
 * Bins: NB = 0x3F81 = 16257.  A score s has key 0 if s is NaN or s <= 0, and min(bits(s) >> 16, 0x3F80) otherwise, where
 * bits is the f32 pattern: the score truncated to bf16, everything from 1.0 on (+inf included) in the last bin.  The
 * lower edge of bin k is the f32 of pattern k << 16.  Integer arithmetic only; 2^-7 relative resolution everywhere.
 * State, owned by the caller and zeroed by the caller ONCE:
 *   hist_tp i32 [T][C1][4][NB], hist_seen i32 [C1][4][NB], anno_total i64 [C1][4].
 *
 * fod_ap_hist_accum: ONE launch over
 *   confs f32 [T][C1][P_total], is_positive u8 [T][C1][P_total], size_categories u8 [C1][4][P_total] (flags 0 or 1),
 *   num_annos i64 [C1][4]
 * for any P_total >= 1.  For slot p of class c the key is that of confs[0][c][p]: both producers write one score for
 * every t, and only t = 0 is read.  With f_s = size_categories[c][s][p]:
 *   hist_seen[c][s][key] += f_s;   hist_tp[t][c][s][key] += is_positive[t][c][p] & f_s;   anno_total[c][s] += num_annos[c][s].
 * A slot whose four flags are 0 (the producers' padding) adds nothing and reads nothing beyond its flags.  The adds are
 * integer atomics on global memory; no float atomics, no scratch.  A bin that would pass 2^31 - 1 is not claimed.
 * FOD_ERR_ARG before any launch: T outside 1..16; C1 < 2; P_total < 1; C1 * ceil(P_total / 256) beyond 2^31 - 1; a NULL
 * operand.
 *
 * fod_ap_hist_finalize: ONE launch, one workgroup per (t, c, s) row, the NB bins walked from the low-score end in chunks
 * with wave-level scans; the state is read only.  Everything from the integers on is f64, each operation rounded once.
 * With A = anno_total[c][s], tp_b = hist_tp[t][c][s][b], se_b = hist_seen[c][s][b] (tp_b <= se_b, as the accumulation
 * leaves them), TP_b / SE_b their sums over the bins of key >= b, and a bin NON-EMPTY iff se_b > 0:
 *   totals i64 [T][C1][4][2] = (TP_0, SE_0): the true positives and the candidates of the row.
 *   ap f64 [T][C1][4] = (sum over b of tp_b * (TP_b / (SE_b + 1e-5))) / A: the reference's mean precision at the true
 *        positives (utils/od_map.py:290-314) taken on bins -- every candidate of a bin is counted before the bin's
 *        precision is taken.  The order of the sum is the kernel's own: within (n + 3) * 2^-53 of any other, n non-empty
 *        bins.
 *   p_b = TP_b / SE_b on non-empty bins (one division); env_b = the maximum of p_b' over the non-empty bins b' <= b.
 *   pr f64 [T][C1][4][101], pr_score f32 [T][C1][4][101]: for i = 0..100, with b the HIGHEST non-empty bin for which
 *        TP_b * 100 >= i * A (compared in i64: no recall is rounded), pr[i] = env_b and pr_score[i] = the lower edge of b;
 *        no such bin: both 0.
 *   ap101 f64 [T][C1][4] = (pr[0] + pr[1] + ... + pr[100]) / 101, summed in that order.
 * A <= 0: ap, ap101, pr and pr_score of the row are NaN (the reference's 0 / 0); totals is still written.
 * Every output element has exactly one writer.
 * FOD_ERR_ARG before any launch: T outside 1..16; C1 < 2; a NULL operand.
 * Not this: equality with the sorted AP where two candidates of a (class, size) row share a bin; COCO's area ranges or
 * maxDets; tracking metrics. */
int fod_ap_hist_accum(const float* confs, const uint8_t* is_positive, const uint8_t* size_categories,
                      const int64_t* num_annos, int T, int C1, long P_total, int* hist_tp, int* hist_seen,
                      int64_t* anno_total, fod_stream_t stream);
int fod_ap_hist_finalize(const int* hist_tp, const int* hist_seen, const int64_t* anno_total, int T, int C1, double* ap,
                         double* ap101, double* pr, float* pr_score, int64_t* totals, fod_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FOD_EXT_H_ */
