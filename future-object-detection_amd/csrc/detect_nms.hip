// Greedy hard NMS over the rows fod_detect_select wrote (include/fod_ext.h: fod_detect_nms has the contract), ONE launch,
// one workgroup per sample, thread j owns row j (wave w owns the 64 rows of block w).
//
// The rule "row j is kept iff no KEPT row i < j suppresses it" is a serial chain over the rows.  It is cut into blocks
// of 64:
//   A. every wave builds its block's 64 x 64 diagonal in parallel: lane i ends up holding word_i, bit j of which says
//      "row 64w+i suppresses row 64w+j" (j > i), one __ballot per i.
//   B. for block w = 0, 1, ...: wave w knows which of its rows earlier blocks suppressed (a register flag per lane), so it
//      resolves its block with scalar work only -- take the lowest row still standing whose word is not empty, strike
//      the rows its word names, go on above it -- and publishes the kept rows as one 64-bit word; after the barrier the
//      waves of LATER blocks take that block's 64 staged rows from LDS, one per lane, walk the word's rows (v_readlane)
//      and raise their lanes' flags.
//   C. positions from the popcounts of the kept words; a kept thread writes its own row -- which it has held in registers
//      since before the first barrier, so every output may alias its input -- and thread r >= survivors writes padding
//      row r.  Every output row has exactly one writer.
// LDS holds what the test needs of a row: box, area and the class that counts, 24 B per row (24.1 KiB at 1024 rows).
// Every access is lane l to row base + l: 16 bytes to consecutive slots or 4 bytes to consecutive dwords, no bank
// conflict.  Inside the loops a row comes out of a lane's registers (v_readlane), not out of LDS.
// No scratch, no atomics, nothing between workgroups; the order of every decision is fixed: deterministic.
#include "det_rows.h"   // fp contract(off) from here on (explained there): the suppression test rounds every operation once

// min / max of a wave-uniform value and a lane's own as ONE instruction.  fminf / fmaxf on a value that came through
// v_readlane cost a second one each (v_max_f32 s, s: the compiler re-quiets a possible signalling NaN); the corners
// that reach the test are finite, so there is nothing to quiet.
FOD_DEVINL float nms_min(float uniform, float own) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "s"(uniform), "v"(own));
  return r;
}
FOD_DEVINL float nms_max(float uniform, float own) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "s"(uniform), "v"(own));
  return r;
}

// `a` (wave-uniform) suppresses `b` (the class condition is the caller's): inter > thr * uni, no division
FOD_DEVINL bool nms_overlaps(const float4 a, const float area_a, const float4 b, const float area_b, const float thr) {
  const float iw = fmaxf(nms_min(a.z, b.z) - nms_max(a.x, b.x), 0.f);
  const float ih = fmaxf(nms_min(a.w, b.w) - nms_max(a.y, b.y), 0.f);
  const float inter = iw * ih;
  const float uni = (area_a + area_b) - inter;
  return inter > thr * uni;
}

__global__ __launch_bounds__(1024) void detect_nms_kernel(
    const float* in_scores, const int32_t* in_labels, const float* in_boxes, const int32_t* in_query,
    const int32_t* in_count, int K, float thr, int class_agnostic, float* out_scores, int32_t* out_labels,
    float* out_boxes, int32_t* out_query, int32_t* out_count, int32_t* out_source) {   // (no __restrict__: they may alias)
  __shared__ float4 s_box[ROWS_MAX];                    // the box the test reads: zeros for a row that takes no part
  __shared__ float s_area[ROWS_MAX];
  __shared__ int s_cls[ROWS_MAX];
  __shared__ unsigned long long s_kept[ROWS_MAX / 64];
  const int b = blockIdx.x, j = threadIdx.x, lane = j & 63, wave = j >> 6;
  const int n = row_count(in_count, b, K);
  const int nblk = (n + 63) >> 6;
  const long row = (long)b * K + j;

  // ---- stage: the row itself stays in registers (it is what gets written), the test's operands go to LDS
  const bool valid = j < n;
  float score = 0.f;
  int label = -1, query = -1;
  float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
  if (valid) {
    score = in_scores[row];
    label = in_labels[row];
    query = in_query[row];
    box = row_box(in_boxes + row * 4);
  }
  // a row with a non-finite coordinate is kept and suppresses nothing: tested here, once, and the test then sees a
  // zero box in its place -- against any box of finite corners that gives inter = 0, and 0 > thr * uni never holds
  // (thr * uni is >= 0 or NaN).  Rows beyond n are zero boxes as well; they are never candidates.
  // (row_finite(box), spelled out: through the helper the two subtractions of the area below stop being one v_pk_add_f32)
  const bool finite = isfinite(box.x) && isfinite(box.y) && isfinite(box.z) && isfinite(box.w);
  const float4 tb = finite ? box : make_float4(0.f, 0.f, 0.f, 0.f);
  const float area = row_area(tb);
  const int cls = class_agnostic ? 0 : label;
  s_box[j] = tb;                                          // (the launch has at most ROWS_MAX threads)
  s_area[j] = area;
  s_cls[j] = cls;
  __syncthreads();

  // ---- A. the diagonal words of this wave's block: row i of the block is lane i's registers, read with v_readlane
  unsigned long long word = 0ull;                        // lane i: the rows of this block that row 64 * wave + i suppresses
  if (wave < nblk) {
    const int last = min(64, n - wave * 64);             // rows of this block that exist
    const unsigned long long live = __ballot(valid);
    for (int i = 0; i + 1 < last; ++i) {
      // (two ballots and scalar ands: one `&&` of the two tests cost a v_cndmask and a second compare per step)
      const unsigned long long w = __ballot(cls == row_lane(cls, i)) &
                                   __ballot(nms_overlaps(row_lane(tb, i), row_lane(area, i), tb, area, thr)) &
                                   live & ~((2ull << i) - 1ull);                      // rows above i only
      if (lane == i) word = w;
    }
  }

  // ---- B. block after block
  bool suppressed = false;                               // by a kept row of an earlier block
  for (int blk = 0; blk < nblk; ++blk) {
    if (wave == blk) {
      // only a row whose word is not empty can strike another one: those that still stand are visited in order, the
      // rest of the block needs no step (none at all where nothing overlaps)
      unsigned long long standing = __ballot(valid && !suppressed), todo = __ballot(word != 0ull);
      while (standing & todo) {
        const int i = __builtin_ctzll(standing & todo);
        standing &= ~row_lane(word, i);                    // bits above i only: row i itself stays
        todo &= ~((2ull << i) - 1ull);
      }
      if (lane == 0) s_kept[blk] = standing;
    }
    __syncthreads();
    if (wave > blk && wave < nblk) {
      // the block's 64 rows, one per lane (consecutive addresses: no bank conflict), then one v_readlane set per kept row:
      // with a broadcast LDS read per kept row instead, the read's latency was the whole time of this loop
      const float4 ob = s_box[blk * 64 + lane];
      const float oa = s_area[blk * 64 + lane];
      const int oc = s_cls[blk * 64 + lane];
      unsigned long long m = row_uniform64(s_kept[blk]), struck = 0ull;
      if (__ballot(valid && !suppressed) == 0ull) m = 0ull;               // nobody left to strike in this wave
      while (m) {
        const int i = __builtin_ctzll(m);
        m &= m - 1;
        struck |= __ballot(cls == row_lane(oc, i)) & __ballot(nms_overlaps(row_lane(ob, i), row_lane(oa, i), tb, area, thr));
      }
      suppressed |= (struck >> lane) & 1ull;
    }
  }

  // ---- C. survivors to the front, padding behind them
  int before = 0, total = 0;
  for (int w = 0; w < nblk; ++w) {
    const int c = __popcll(s_kept[w]);
    before += w < wave ? c : 0;
    total += c;
  }
  const bool keep = wave < nblk && ((s_kept[wave] >> lane) & 1ull);
  if (keep) {
    const long o = (long)b * K + before + __popcll(s_kept[wave] & ((1ull << lane) - 1ull));
    out_scores[o] = score;
    out_labels[o] = label;
    out_query[o] = query;
    row_put(out_boxes + o * 4, box);
    if (out_source) out_source[o] = j;
  }
  if (j >= total && j < K) {
    out_scores[row] = 0.f;
    out_labels[row] = -1;
    out_query[row] = -1;
    row_put(out_boxes + row * 4, make_float4(0.f, 0.f, 0.f, 0.f));
    if (out_source) out_source[row] = -1;
  }
  if (j == 0) out_count[b] = total;
}

extern "C" int fod_detect_nms(const float* scores, const int* labels, const float* boxes, const int* query,
                              const int* count, int B, int K, float iou_threshold, int class_agnostic,
                              float* out_scores, int* out_labels, float* out_boxes, int* out_query, int* out_count,
                              int* out_source, hipStream_t stream) {
  FOD_REQUIRE(K >= 1 && K <= ROWS_MAX, "detect_nms: K=%d is outside 1..%d", K, ROWS_MAX);
  FOD_REQUIRE(B >= 1, "detect_nms: B=%d samples, at least 1 expected", B);
  FOD_REQUIRE(iou_threshold >= 0.f && iou_threshold <= 1.f, "detect_nms: iou_threshold=%g is outside [0, 1]",
              (double)iou_threshold);
  FOD_REQUIRE(scores && labels && boxes && query && count && out_scores && out_labels && out_boxes && out_query &&
                  out_count, "detect_nms: null operand (only out_source may be NULL)");
  const int threads = ((K + 63) / 64) * 64;              // thread j owns row j
  hipLaunchKernelGGL(detect_nms_kernel, dim3(B), dim3(threads), 0, stream, scores, labels, boxes, query, count, K,
                     iou_threshold, class_agnostic != 0, out_scores, out_labels, out_boxes, out_query, out_count,
                     out_source);
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}
