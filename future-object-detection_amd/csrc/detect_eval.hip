// AP bookkeeping over DETECTION ROWS (include/fod_ext.h: fod_detect_od_map has the contract): the greedy true / false
// positive assignment of od_map_kernel (csrc/loss.hip), with the ranked candidates taken from the rows fod_detect_select /
// fod_detect_nms left instead of from a dense score tensor.  ONE launch, one workgroup per (class, sample), T waves:
//   1. all threads stage the sample's annotations (box, clamped area, "may be claimed by this class") and the rows' keys
//      (the label, for the generic class the query) in LDS;
//   2. the candidates of the class are compacted in row order: a ballot per wave, the waves' counts through LDS, 64 * T
//      rows per round -- an ordered block-wide prefix; only the first P positions are kept;
//   3. all threads stage the candidates (box, clamped area, score, finite) and write what does not depend on the
//      threshold: the size flags, and for slots behind the last candidate the padding;
//   4. wave t walks the candidates for threshold t.  Lane l owns the annotations l, l + 64, ...: their free bits are one
//      word of LDS per lane (read and written by that lane only: no hazard, no barrier), the arg-max goes across the lanes
//      with xor shuffles, after which every lane knows the winner and the owner strikes it.  Lane k % 64 collects the
//      decision of candidate k, so confs / is_positive leave as whole coalesced rows at the end;
//   5. the workgroups of sample 0 count their class's annotations over ALL samples: one writer per num_annos row.
// Every output element has exactly one writer, nothing is accumulated in memory, no scratch, no atomics, nothing between
// workgroups: the outputs need no initialisation and two launches give equal bits.
#include "det_rows.h"   // fp contract(off) from here on (explained there): the IoU is od_map_kernel's, operation for operation

constexpr int DE_MAX_T = 16;                           // waves; rows and annotation slots: ROWS_MAX

__global__ __launch_bounds__(1024) void detect_od_map_kernel(
    const float* __restrict__ scores, const int32_t* __restrict__ labels, const float* __restrict__ boxes,
    const int32_t* __restrict__ query, const int32_t* __restrict__ count, const float* __restrict__ ab,
    const int64_t* __restrict__ ac, const int64_t* __restrict__ aa, float* __restrict__ confs,
    uint8_t* __restrict__ is_pos, uint8_t* __restrict__ sizes, long long* __restrict__ num_annos, int B, int K, int N,
    int C1, int P, float H, float W) {
  __shared__ float4 s_abox[ROWS_MAX];                   // annotations: zeros where the box is not finite
  __shared__ float4 s_cbox[ROWS_MAX];                   // candidates, in rank order
  __shared__ float s_aarea[ROWS_MAX];
  __shared__ float s_carea[ROWS_MAX];
  __shared__ float s_cscore[ROWS_MAX];
  __shared__ int s_key[ROWS_MAX];                       // per row: the label, for the generic class the query
  __shared__ unsigned s_free[DE_MAX_T * 64];            // per wave and lane: bit r = annotation lane + 64 r is free
  __shared__ unsigned short s_cand[ROWS_MAX];           // candidate k's row
  __shared__ unsigned char s_avail[ROWS_MAX];           // free at the start
  __shared__ unsigned char s_cfin[ROWS_MAX];            // candidate k's box is finite
  __shared__ int s_wcnt[DE_MAX_T];
  __shared__ long long s_cnt[DE_MAX_T][4];
  const int c = blockIdx.x % C1, b = blockIdx.x / C1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, T = nthreads >> 6;
  const bool generic = c == C1 - 1;
  const int n = row_count(count, b, K);
  const float s0 = (float)((1.0 / 24) * (1.0 / 64) * (double)H * (double)W);     // od_map_kernel's delimiters
  const float s1 = (float)((1.0 / 4) * (1.0 / 12) * (double)H * (double)W);
  const long slots = (long)B * P;

  // ---- 1. annotations and keys
  for (int a = tid; a < N; a += nthreads) {
    const long i = (long)b * N + a;
    const float4 box = row_box(ab + i * 4);
    const bool fin = row_finite(box);                    // tested before any min / max sees the value
    const float4 tb = fin ? box : make_float4(0.f, 0.f, 0.f, 0.f);
    s_abox[a] = tb;
    s_aarea[a] = row_area(tb);
    s_avail[a] = fin && aa[i] == 1 && (generic || ac[i] == c);
  }
  for (int j = tid; j < n; j += nthreads) s_key[j] = generic ? query[(long)b * K + j] : labels[(long)b * K + j];
  __syncthreads();

  // ---- 2. the class's candidates, compacted in row order; positions from P on are cut
  int total = 0;                                         // (block-uniform)
  for (int base = 0; base < n && total < P; base += nthreads) {
    const int j = base + tid;
    bool cand = false;
    if (!generic) {
      cand = j < n && s_key[j] == c;
    } else {
      // the first row of its query: every lane of the wave reads the same s_key[i] (a broadcast)
      const int first = base + wave * 64;                 // (a wave wholly beyond n walks nothing)
      const int last = first < n ? min(n, first + 64) : 0, q = j < n ? s_key[j] : 0;
      bool seen = false;
      for (int i = 0; i + 1 < last; ++i) seen |= (s_key[i] == q) && (i < j);
      cand = j < n && !seen;
    }
    const unsigned long long word = __ballot(cand);
    if (lane == 0) s_wcnt[wave] = __popcll(word);
    __syncthreads();
    int before = total;
    for (int w = 0; w < T; ++w) {
      const int cnt = s_wcnt[w];
      before += w < wave ? cnt : 0;
      total += cnt;
    }
    const int pos = before + __popcll(word & ((1ull << lane) - 1ull));
    if (cand && pos < P) s_cand[pos] = (unsigned short)j;
    __syncthreads();                                     // s_wcnt is written again in the next round
  }
  const int ncand = min(total, P);

  // ---- 3. the candidates themselves; size flags and padding (nothing here depends on the threshold)
  for (int k = tid; k < P; k += nthreads) {
    const long o = (long)b * P + k;
    unsigned char f1 = 0, f2 = 0, f3 = 0;
    if (k < ncand) {
      const long row = (long)b * K + s_cand[k];
      const float4 box = row_box(boxes + row * 4);
      const bool fin = row_finite(box);
      s_cbox[k] = box;
      s_carea[k] = row_area(box);
      s_cscore[k] = scores[row];
      s_cfin[k] = fin;
      if (fin) {
        const float area = (box.z - box.x) * (box.w - box.y);      // unclamped, as od_map_kernel's flags
        f1 = area <= s0;
        f2 = (s0 < area) && (area <= s1);
        f3 = s1 < area;
      }
    }
    sizes[((long)c * 4 + 0) * slots + o] = k < ncand;
    sizes[((long)c * 4 + 1) * slots + o] = f1;
    sizes[((long)c * 4 + 2) * slots + o] = f2;
    sizes[((long)c * 4 + 3) * slots + o] = f3;
  }
  {
    unsigned mask = 0u;
    for (int r = 0; r * 64 < N; ++r) {
      const int a = lane + 64 * r;
      if (a < N && s_avail[a]) mask |= 1u << r;
    }
    s_free[tid] = mask;                                  // the wave's own copy
  }
  __syncthreads();

  // ---- 4. wave `wave` walks the candidates for its threshold
  {
    const int t = wave;
    const float thr = (float)(0.5 + (double)t * 0.05);   // od_map_kernel's thresholds
    unsigned mine = 0u;                                  // bit r: candidate lane + 64 r is positive
    for (int k = 0; k < ncand; ++k) {
      bool positive = false;
      if (s_cfin[k]) {                                   // (wave-uniform) a non-finite row claims nothing
        const float4 p = s_cbox[k];
        const float area1 = s_carea[k];
        const unsigned freem = s_free[tid];
        float best = 0.f;
        int best_a = 0x7fffffff;
        for (int r = 0; r * 64 < N; ++r) {
          const int a = lane + 64 * r;
          float iou = 0.f;
          if (a < N && ((freem >> r) & 1u)) {
            const float4 q = s_abox[a];
            // row_inter(p, q), spelled out: through the helper the compiler allocates this loop's registers differently
            const float inter = fmaxf(fminf(p.z, q.z) - fmaxf(p.x, q.x), 0.f) * fmaxf(fminf(p.w, q.w) - fmaxf(p.y, q.y), 0.f);
            iou = (inter + 1e-7f) / (area1 + s_aarea[a] - inter + 1e-7f);
          }
          if (a < N && (iou > best || (iou == best && a < best_a))) { best = iou; best_a = a; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float ob = __shfl_xor(best, o);
          const int oa = __shfl_xor(best_a, o);
          if (ob > best || (ob == best && oa < best_a)) { best = ob; best_a = oa; }
        }
        positive = best >= thr;                          // every lane holds the winner
        if (positive && (best_a & 63) == lane) s_free[tid] = freem & ~(1u << (best_a >> 6));
      }
      if ((k & 63) == lane && positive) mine |= 1u << (k >> 6);
    }
    const long o = ((long)t * C1 + c) * slots + (long)b * P;
    for (int r = 0; r * 64 < P; ++r) {
      const int k = lane + 64 * r;
      if (k < P) {
        confs[o + k] = k < ncand ? s_cscore[k] : 0.f;
        is_pos[o + k] = (mine >> r) & 1u;
      }
    }
  }

  // ---- 5. annotation counts of the class, over all samples: the workgroups of sample 0
  if (b == 0) {
    long long cnt[4] = {0, 0, 0, 0};
    for (long i = tid; i < (long)B * N; i += nthreads) {
      if (aa[i] != 1 || !(generic || ac[i] == c)) continue;
      const float4 box = row_box(ab + i * 4);
      cnt[0] += 1;
      if (row_finite(box)) {                             // a non-finite annotation counts in column 0 only
        const float area = (box.z - box.x) * (box.w - box.y);
        cnt[1] += area <= s0;
        cnt[2] += (s0 < area) && (area <= s1);
        cnt[3] += s1 < area;
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      long long sum = cnt[s];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
      if (lane == 0) s_cnt[wave][s] = sum;
    }
    __syncthreads();
    if (tid < 4) {
      long long sum = 0;
      for (int w = 0; w < T; ++w) sum += s_cnt[w][tid];
      num_annos[c * 4 + tid] = sum;
    }
  }
}

extern "C" int fod_detect_od_map(const float* scores, const int* labels, const float* boxes, const int* query,
                                 const int* count, const float* anno_boxes, const int64_t* anno_classes,
                                 const int64_t* anno_active, float* confs, uint8_t* is_positive,
                                 uint8_t* size_categories, int64_t* num_annos, int B, int K, int N, int C, int P, int T,
                                 float img_h, float img_w, hipStream_t stream) {
  FOD_REQUIRE(B >= 1, "detect_od_map: B=%d samples, at least 1 expected", B);
  FOD_REQUIRE(K >= 1 && K <= ROWS_MAX, "detect_od_map: K=%d is outside 1..%d", K, ROWS_MAX);
  FOD_REQUIRE(N >= 1 && N <= ROWS_MAX, "detect_od_map: N=%d is outside 1..%d", N, ROWS_MAX);
  FOD_REQUIRE(P >= 1 && P <= K, "detect_od_map: P=%d is outside 1..K=%d", P, K);
  FOD_REQUIRE(T >= 1 && T <= DE_MAX_T, "detect_od_map: T=%d is outside 1..%d", T, DE_MAX_T);
  FOD_REQUIRE(C >= 1, "detect_od_map: C=%d classes, at least 1 expected", C);
  FOD_REQUIRE((long)(C + 1L) * B <= 0x7fffffffL, "detect_od_map: (C + 1) * B = %ld workgroups", (long)(C + 1L) * B);
  FOD_REQUIRE(scores && labels && boxes && query && count && anno_boxes && anno_classes && anno_active && confs &&
                  is_positive && size_categories && num_annos, "detect_od_map: null operand");
  hipLaunchKernelGGL(detect_od_map_kernel, dim3((unsigned)((C + 1) * B)), dim3(T * 64), 0, stream, scores, labels, boxes,
                     query, count, anno_boxes, anno_classes, anno_active, confs,
                     is_positive, size_categories, (long long*)num_annos, B, K, N, C + 1, P, img_h, img_w);
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}
