// Identities across calls (include/fod_ext.h: fod_track_update has the contract): the rows of one call claim the tracks
// the caller keeps, unclaimed tracks age and retire, unmatched rows start new ones.  ONE launch, one workgroup per
// sample; thread j owns row j, thread s owns slot s (the launch has max(K, S) threads, rounded up to whole waves).
//   0. stage: a thread keeps its row and its slot in registers; the predicted box, its area and the class that counts go
//      to LDS per slot, the row's box and class per row (24 B each), the claimable slots as one ballot word per wave.
//   A. every row finds its best slot as if nothing were claimed, in parallel: a wave takes 64 slots into its lanes' registers
//      and walks the claimable ones with v_readlane, as fod_detect_nms walks its kept rows.  A row whose best IoU is below
//      the threshold can never match -- claims only remove options -- and takes no part in B.
//   B. the serial chain, inside wave 0, no barrier per row: lane l owns the slots l, l + 64, ... and keeps their claimed
//      bits in one register.  A row whose best slot of A is still unclaimed is decided by scalar work (that slot is then
//      also the best of the unclaimed ones); only a row whose best was taken recomputes its arg-max over the unclaimed
//      slots, 16 per lane at S = 1024, and reduces it across the lanes with xor shuffles.
//   C. slots: update, age, clear -- in registers.  The ranks of the free slots and of the rows to be born are ballots and
//      popcounts, the waves' counts go through LDS; the r-th free slot is published for the r-th newborn row.
//   D. writes.  A matched slot writes its row's outputs; a row writes its own outputs otherwise, and the state of the slot
//      it is born in.  A slot that was cleared and is born in again in the same call is written by the newborn row only:
//      every element has exactly one writer.
// No scratch, no atomics, nothing between workgroups; the order of every decision is fixed: deterministic.
#include "det_rows.h"   // fp contract(off) from here on (explained there): `box + vel * gap` would become one v_fma_f32

// the header's IoU of a row `a` and a predicted box `q`; `inter` comes back as well (the match needs inter > 0).
// To be called by all lanes of a wave together.  The correctly rounded division is most of the work, and most pairs do not
// overlap: where inter is +0 (or NaN, and uni with it) the header's expression is +0 whatever uni is, so a wave in which no
// lane has inter > 0 skips the division -- the same bits, a wave-uniform branch.
FOD_DEVINL float trk_iou(const float4 a, const float area_a, const float4 q, const float area_q, float& inter) {
  inter = row_inter(a, q);
  float iou = 0.f;
  if (__ballot(inter > 0.f) != 0ull) {
    const float uni = (area_a + area_q) - inter;
    iou = (inter > 0.f && uni > 0.f) ? inter / uni : 0.f;
  }
  return iou;
}

__global__ __launch_bounds__(1024) void track_update_kernel(
    const float* __restrict__ scores, const int32_t* __restrict__ labels, const float* __restrict__ boxes,
    const int32_t* __restrict__ count, float* __restrict__ trk_boxes, float* __restrict__ trk_vel,
    int32_t* __restrict__ trk_meta, float* __restrict__ trk_scores, int32_t* __restrict__ next_id,
    int32_t* __restrict__ out_track, int32_t* __restrict__ out_hits, int32_t* __restrict__ out_slot, int K, int S,
    float thr, float birth_score, int max_misses, int class_agnostic, int motion) {
  __shared__ float4 s_pbox[ROWS_MAX];                   // slots: the predicted box, zeros where it cannot be claimed
  __shared__ float4 s_rbox[ROWS_MAX];                   // rows: the box, zeros where it is not finite or beyond n
  __shared__ float s_parea[ROWS_MAX];
  __shared__ int s_pcls[ROWS_MAX];
  __shared__ int s_rcls[ROWS_MAX];
  __shared__ int s_rbest[ROWS_MAX];                     // rows: A leaves best slot | matched << 16 (or -1), B the claimed slot (or -1)
  __shared__ int s_smatch[ROWS_MAX];                    // slots: the row that claimed it, or -1
  __shared__ int s_list[ROWS_MAX];                      // the r-th free slot
  __shared__ unsigned long long s_availw[ROWS_MAX / 64];   // per 64 slots: claimable
  __shared__ unsigned long long s_candw[ROWS_MAX / 64];    // per 64 rows: takes part in B
  __shared__ int s_fcnt[ROWS_MAX / 64], s_bcnt[ROWS_MAX / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
  const int n = row_count(count, b, K);
  const int first_id = next_id[b];                       // (read by every thread before the first barrier; written after the last)
  const int nsblk = (S + 63) >> 6, nrblk = (n + 63) >> 6;
  const long row = (long)b * K + tid, slot = (long)b * S + tid;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

  // ---- 0. stage
  int id = -1, slabel = -1, hits = 0, misses = 0;
  float4 sbox = zero4, svel = zero4, pbox = zero4;
  float sscore = 0.f, gap = 1.f;
  bool claimable = false;
  if (tid < S) id = trk_meta[slot * 4];
  bool live = id >= 0;                                   // the other fields of a free slot are never read
  if (live) {
    slabel = trk_meta[slot * 4 + 1];
    hits = trk_meta[slot * 4 + 2];
    misses = trk_meta[slot * 4 + 3];
    sbox = row_box(trk_boxes + slot * 4);
    svel = row_box(trk_vel + slot * 4);
    gap = (float)(misses + 1);
    pbox = motion ? make_float4(sbox.x + svel.x * gap, sbox.y + svel.y * gap, sbox.z + svel.z * gap, sbox.w + svel.w * gap)
                  : sbox;
    claimable = row_finite(pbox);
  }
  if (!claimable) pbox = zero4;
  s_pbox[tid] = pbox;                                    // (the launch has at most ROWS_MAX threads)
  s_parea[tid] = row_area(pbox);
  s_pcls[tid] = class_agnostic ? 0 : slabel;
  s_smatch[tid] = -1;
  {
    const unsigned long long w = __ballot(claimable);
    if (lane == 0) s_availw[wave] = w;
  }
  float score = 0.f;
  int label = -1;
  float4 box = zero4;
  if (tid < n) {
    score = scores[row];
    label = labels[row];
    box = row_box(boxes + row * 4);
  }
  const bool fin = tid < n && row_finite(box);          // tested here, once: a row that fails it takes no part at all
  const float4 rb = fin ? box : zero4;
  const float rarea = row_area(rb);
  const int rcls = class_agnostic ? 0 : label;
  s_rbox[tid] = rb;
  s_rcls[tid] = rcls;
  __syncthreads();

  // ---- A. every row's best slot with nothing claimed: 64 slots in the lanes' registers, walked with v_readlane
  {
    float best = -1.f, binter = 0.f;                     // (an IoU is never negative and never NaN)
    int bslot = -1;
    if (__ballot(fin) != 0ull) {
      for (int blk = 0; blk < nsblk; ++blk) {
        unsigned long long m = row_uniform64(s_availw[blk]);
        if (m == 0ull) continue;
        const float4 ob = s_pbox[blk * 64 + lane];
        const float oa = s_parea[blk * 64 + lane];
        const int oc = s_pcls[blk * 64 + lane];
        while (m) {
          const int i = __builtin_ctzll(m);
          m &= m - 1;
          float inter;
          const float iou = trk_iou(rb, rarea, row_lane(ob, i), row_lane(oa, i), inter);
          if (rcls == row_lane(oc, i) && iou > best) {   // ascending slots, strictly greater: ties stay with the lowest
            best = iou;
            binter = inter;
            bslot = blk * 64 + i;
          }
        }
      }
    }
    const bool cand = fin && bslot >= 0 && best >= thr;
    const bool matched = cand && binter > 0.f;
    s_rbest[tid] = cand ? (bslot | ((int)matched << 16)) : -1;
    const unsigned long long w = __ballot(cand);
    if (lane == 0) s_candw[wave] = w;
  }
  __syncthreads();

  // ---- B. the claim walk, wave 0
  if (wave == 0) {
    unsigned claimed = 0u;                               // bit r: slot lane + 64 r is claimed
    for (int w = 0; w < nrblk; ++w) {
      unsigned long long m = row_uniform64(s_candw[w]);
      if (m == 0ull) continue;
      const int packed = s_rbest[w * 64 + lane];
      const float4 qb = s_rbox[w * 64 + lane];
      const int qc = s_rcls[w * 64 + lane];
      int mine = -1;                                     // lane i: the slot row 64 w + i claimed
      while (m) {
        const int i = __builtin_ctzll(m);
        m &= m - 1;
        const int p = row_lane(packed, i), bs = p & 0xffff;
        int got = -1;
        if (((row_lane((int)claimed, bs & 63) >> (bs >> 6)) & 1) == 0) {
          if (p >> 16) got = bs;                          // its best of A stands: also the best of what is left
        } else {
          const float4 q = row_lane(qb, i);
          const float qarea = row_area(q);
          const int cls = row_lane(qc, i);
          float best = -1.f, binter = 0.f;
          int bslot = 0x7fffffff;
          for (int r = 0; r < nsblk; ++r) {
            const int a = lane + 64 * r;                  // (below 64 * nsblk: every such entry was staged)
            const bool open = ((s_availw[r] >> lane) & 1ull) && !((claimed >> r) & 1u) && s_pcls[a] == cls;
            float inter;
            const float iou = trk_iou(q, qarea, s_pbox[a], s_parea[a], inter);
            if (open && iou > best) {
              best = iou;
              binter = inter;
              bslot = a;
            }
          }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o), oi = __shfl_xor(binter, o);
            const int os = __shfl_xor(bslot, o);
            if (ob > best || (ob == best && os < bslot)) {
              best = ob;
              binter = oi;
              bslot = os;
            }
          }
          if (bslot != 0x7fffffff && binter > 0.f && best >= thr) got = bslot;     // every lane holds the winner
        }
        if (got >= 0 && (got & 63) == lane) {
          claimed |= 1u << (got >> 6);
          s_smatch[got] = w * 64 + i;
        }
        if (lane == i) mine = got;
      }
      s_rbest[w * 64 + lane] = mine;                     // (rows that took no part hold -1 already, here and elsewhere)
    }
  }
  __syncthreads();

  // ---- C. slots in registers; ranks of the free slots and of the rows to be born
  const int mrow = tid < S ? s_smatch[tid] : -1;         // slot: the row that claimed it
  const int mslot = s_rbest[tid];                         // row: the slot it claimed
  bool dirty = false;                                    // the slot's state changed
  if (live) {
    dirty = true;
    if (mrow >= 0) {
      const float4 nb = s_rbox[mrow];                    // (a claiming row is finite: this is its box, bit for bit)
      svel = motion ? make_float4((nb.x - sbox.x) / gap, (nb.y - sbox.y) / gap, (nb.z - sbox.z) / gap, (nb.w - sbox.w) / gap)
                    : zero4;
      sbox = nb;
      sscore = scores[(long)b * K + mrow];
      slabel = labels[(long)b * K + mrow];
      hits += 1;
      misses = 0;
    } else {
      sscore = trk_scores[slot];
      misses += 1;
      if (misses > max_misses) {
        live = false;
        id = -1, slabel = -1, hits = 0, misses = 0;
        sbox = zero4, svel = zero4, sscore = 0.f;
      }
    }
  }
  const bool is_free = tid < S && !live;                 // as judged after the clearing
  const bool born = fin && mslot < 0 && score >= birth_score;     // a candidate, that is (a NaN score never qualifies)
  const unsigned long long fw = __ballot(is_free), bw = __ballot(born);
  if (lane == 0) {
    s_fcnt[wave] = __popcll(fw);
    s_bcnt[wave] = __popcll(bw);
  }
  __syncthreads();
  int frank = 0, brank = 0, nfree = 0, ncand = 0;
  for (int w = 0; w < nwaves; ++w) {
    const int fc = s_fcnt[w], bc = s_bcnt[w];
    frank += w < wave ? fc : 0;
    brank += w < wave ? bc : 0;
    nfree += fc;
    ncand += bc;
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  frank += __popcll(fw & below);
  brank += __popcll(bw & below);
  const int nborn = min(nfree, ncand);
  if (is_free && frank < nborn) s_list[frank] = tid;
  __syncthreads();

  // ---- D. writes: every element by exactly one thread
  if (dirty && !(is_free && frank < nborn)) {            // (a cleared slot that is born in again: the newborn row writes it)
    row_put(trk_boxes + slot * 4, sbox);
    row_put(trk_vel + slot * 4, svel);
    trk_meta[slot * 4 + 0] = id;
    trk_meta[slot * 4 + 1] = slabel;
    trk_meta[slot * 4 + 2] = hits;
    trk_meta[slot * 4 + 3] = misses;
    trk_scores[slot] = sscore;
  }
  if (live && mrow >= 0) {                               // the matched row's outputs
    const long o = (long)b * K + mrow;
    out_track[o] = id;
    out_hits[o] = hits;
    if (out_slot) out_slot[o] = tid;
  }
  if (tid < K && mslot < 0) {
    int t = -1, h = 0, s = -1;
    if (born && brank < nborn) {
      s = s_list[brank];
      t = first_id + brank;
      h = 1;
      const long o = (long)b * S + s;
      row_put(trk_boxes + o * 4, box);
      row_put(trk_vel + o * 4, zero4);
      trk_meta[o * 4 + 0] = t;
      trk_meta[o * 4 + 1] = label;
      trk_meta[o * 4 + 2] = 1;
      trk_meta[o * 4 + 3] = 0;
      trk_scores[o] = score;
    }
    out_track[row] = t;
    out_hits[row] = h;
    if (out_slot) out_slot[row] = s;
  }
  if (tid == 0) next_id[b] = first_id + nborn;
}

extern "C" int fod_track_update(const float* scores, const int* labels, const float* boxes, const int* count, int B, int K,
                                float* trk_boxes, float* trk_vel, int* trk_meta, float* trk_scores, int* next_id, int S,
                                float iou_threshold, float birth_score, int max_misses, int class_agnostic, int motion,
                                int* out_track, int* out_hits, int* out_slot, hipStream_t stream) {
  FOD_REQUIRE(K >= 1 && K <= ROWS_MAX, "track_update: K=%d is outside 1..%d", K, ROWS_MAX);
  FOD_REQUIRE(S >= 1 && S <= ROWS_MAX, "track_update: S=%d is outside 1..%d", S, ROWS_MAX);
  FOD_REQUIRE(B >= 1, "track_update: B=%d samples, at least 1 expected", B);
  FOD_REQUIRE(iou_threshold >= 0.f && iou_threshold <= 1.f, "track_update: iou_threshold=%g is outside [0, 1]",
              (double)iou_threshold);
  FOD_REQUIRE(max_misses >= 0, "track_update: max_misses=%d is negative", max_misses);
  FOD_REQUIRE(scores && labels && boxes && count && trk_boxes && trk_vel && trk_meta && trk_scores && next_id &&
                  out_track && out_hits, "track_update: null operand (only out_slot may be NULL)");
  const int threads = ((max(K, S) + 63) / 64) * 64;      // thread j owns row j, thread s owns slot s
  hipLaunchKernelGGL(track_update_kernel, dim3(B), dim3(threads), 0, stream, scores, labels, boxes, count, trk_boxes,
                     trk_vel, trk_meta, trk_scores, next_id, out_track, out_hits, out_slot, K, S, iou_threshold,
                     birth_score, max_misses, class_agnostic != 0, motion != 0);
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}
