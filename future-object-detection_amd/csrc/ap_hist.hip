// Streaming AP (include/fod_ext.h: fod_ap_hist_accum / fod_ap_hist_finalize have the contract): the four tensors of the AP
// bookkeeping (fod_od_map, fod_detect_od_map) are folded into INTEGER histograms over score bins, and both AP definitions,
// the precision / recall curve and the operating point come out of one finalising launch.
//   accumulate: one thread per (class, slot).  It reads the slot's four size flags; a slot whose flags are all 0 (padding)
//     touches nothing else.  Any other slot forms its bin from confs[0][c][p] and adds 1 with integer atomics on global
//     memory: exact sums, so the state does not depend on the arrival order and two runs give equal bits.
//   finalise: one workgroup of 256 per (t, c, s) row.  Pass 1 sums the row (TP, SE); pass 2 walks the bins from the
//     LOW-score end in chunks of 256 -- bin = chunk * 256 + thread, coalesced -- with wave-level scans: the counts below a
//     bin (so TP_b = TP - below), and the running maximum of the precision (COCO's envelope).  A bin with tp_b > 0 knows
//     from two integers which of the 101 recall points it answers: no search, no NB-sized array in LDS.
// No float atomics, no scratch; every element of finalise's outputs has one writer.
#include "common.h"

// every f64 operation below is rounded once (pr is ONE division of two exact integers): nothing here may contract
#pragma clang fp contract(off)

constexpr int AH_NB = 0x3F81;                           // bins: bf16 patterns 0 .. 0x3F80 (1.0), everything above clamped
constexpr int AH_MAX_T = 16, AH_THREADS = 256, AH_WAVES = AH_THREADS / 64, AH_POINTS = 101;

FOD_DEVINL int ah_key(const float s) {
  if (!(s > 0.f)) return 0;                             // NaN, zero, negative
  return min((int)(__float_as_uint(s) >> 16), AH_NB - 1);
}

__global__ __launch_bounds__(AH_THREADS) void ap_hist_accum_kernel(
    const float* __restrict__ confs, const uint8_t* __restrict__ is_pos, const uint8_t* __restrict__ sizes,
    const long long* __restrict__ num_annos, int* __restrict__ hist_tp, int* __restrict__ hist_seen,
    unsigned long long* __restrict__ anno_total, int T, int C1, long P, int nblk) {
  const int c = blockIdx.x / nblk, pb = blockIdx.x % nblk, tid = threadIdx.x;
  if (pb == 0 && tid < 4) atomicAdd(anno_total + c * 4 + tid, (unsigned long long)num_annos[c * 4 + tid]);
  const long p = (long)pb * AH_THREADS + tid;
  if (p >= P) return;
  bool f[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) f[s] = sizes[((size_t)c * 4 + s) * P + p] != 0;
  if (!(f[0] || f[1] || f[2] || f[3])) return;          // padding: nothing but its flags is read
  const int key = ah_key(confs[(size_t)c * P + p]);     // t = 0: both producers write one score for every t
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (f[s]) atomicAdd(hist_seen + ((size_t)c * 4 + s) * AH_NB + key, 1);
  for (int t = 0; t < T; ++t) {
    if (is_pos[((size_t)t * C1 + c) * P + p] == 0) continue;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (f[s]) atomicAdd(hist_tp + (((size_t)t * C1 + c) * 4 + s) * AH_NB + key, 1);
  }
}

FOD_DEVINL long long ah_wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(AH_THREADS) void ap_hist_finalize_kernel(
    const int* __restrict__ hist_tp, const int* __restrict__ hist_seen, const long long* __restrict__ anno_total,
    double* __restrict__ ap, double* __restrict__ ap101, double* __restrict__ pr, float* __restrict__ pr_score,
    long long* __restrict__ totals, int C1) {
  __shared__ long long s_wtp[2][AH_WAVES], s_wse[2][AH_WAVES];
  __shared__ double s_wmax[2][AH_WAVES], s_wap[AH_WAVES];
  __shared__ double s_pr[AH_POINTS];
  __shared__ float s_sc[AH_POINTS];
  const int row = blockIdx.x, cs = row % (C1 * 4);       // row = (t * C1 + c) * 4 + s
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* ht = hist_tp + (size_t)row * AH_NB;
  const int* hs = hist_seen + (size_t)cs * AH_NB;
  const long long A = anno_total[cs];

  // ---- pass 1: the row's totals
  long long tp_tot = 0, se_tot = 0;
  for (int b = tid; b < AH_NB; b += AH_THREADS) {
    tp_tot += ht[b];
    se_tot += hs[b];
  }
  tp_tot = ah_wave_sum(tp_tot);
  se_tot = ah_wave_sum(se_tot);
  if (lane == 0) {
    s_wtp[1][wave] = tp_tot;                             // (pass 2 starts with buffer 0)
    s_wse[1][wave] = se_tot;
  }
  if (tid < AH_POINTS) {
    s_pr[tid] = 0.0;
    s_sc[tid] = 0.f;
  }
  __syncthreads();
  tp_tot = se_tot = 0;
#pragma unroll
  for (int w = 0; w < AH_WAVES; ++w) {
    tp_tot += s_wtp[1][w];
    se_tot += s_wse[1][w];
  }
  if (tid == 0) {
    totals[(size_t)row * 2 + 0] = tp_tot;
    totals[(size_t)row * 2 + 1] = se_tot;
  }
  if (A <= 0) {                                          // (block-uniform) no annotation: the reference's 0 / 0
    const double nan = __builtin_nan("");
    if (tid == 0) ap[row] = ap101[row] = nan;
    if (tid < AH_POINTS) {
      pr[(size_t)row * AH_POINTS + tid] = nan;
      pr_score[(size_t)row * AH_POINTS + tid] = __builtin_nanf("");
    }
    return;
  }

  // ---- pass 2: from the low-score end
  long long below_tp = 0, below_se = 0;                  // the counts of all earlier chunks (block-uniform)
  double env_before = -1.0, ap_acc = 0.0;                // the envelope of all earlier chunks; -1: no non-empty bin yet
  for (int base = 0, par = 0; base < AH_NB; base += AH_THREADS, par ^= 1) {
    const int b = base + tid;
    const long long tp = b < AH_NB ? ht[b] : 0, se = b < AH_NB ? hs[b] : 0;
    long long itp = tp, ise = se;                         // inclusive scans inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long a = __shfl_up(itp, o), c2 = __shfl_up(ise, o);
      if (lane >= o) { itp += a; ise += c2; }
    }
    if (lane == 63) { s_wtp[par][wave] = itp; s_wse[par][wave] = ise; }
    __syncthreads();
    long long btp = below_tp + (itp - tp), bse = below_se + (ise - se);
#pragma unroll
    for (int w = 0; w < AH_WAVES; ++w) {
      const long long a = s_wtp[par][w], c2 = s_wse[par][w];
      if (w < wave) { btp += a; bse += c2; }
      below_tp += a;
      below_se += c2;
    }
    const long long TPb = tp_tot - btp, SEb = se_tot - bse;   // inclusive sums over the bins of key >= b
    const double p = se > 0 ? (double)TPb / (double)SEb : -1.0;
    double env = p;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double a = __shfl_up(env, o);
      if (lane >= o) env = fmax(env, a);
    }
    if (lane == 63) s_wmax[par][wave] = env;
    __syncthreads();
    env = fmax(env, env_before);
#pragma unroll
    for (int w = 0; w < AH_WAVES; ++w) {
      const double a = s_wmax[par][w];
      if (w < wave) env = fmax(env, a);
      env_before = fmax(env_before, a);
    }
    if (se > 0) {
      const float edge = __uint_as_float((unsigned)b << 16);
      if (SEb == se) { s_pr[0] = env; s_sc[0] = edge; }   // the highest non-empty bin answers recall 0
      if (tp > 0) {
        ap_acc += (double)tp * ((double)TPb / ((double)SEb + 1e-5));
        const long long lo = max((TPb - tp) * 100 / A + 1, 1ll), hi = min(TPb * 100 / A, (long long)(AH_POINTS - 1));
        for (long long i = lo; i <= hi; ++i) { s_pr[i] = env; s_sc[i] = edge; }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ap_acc += __shfl_xor(ap_acc, o);
  if (lane == 0) s_wap[wave] = ap_acc;
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int w = 0; w < AH_WAVES; ++w) sum += s_wap[w];
    ap[row] = sum / (double)A;
    sum = 0.0;
    for (int i = 0; i < AH_POINTS; ++i) sum += s_pr[i];
    ap101[row] = sum / 101.0;
  }
  if (tid < AH_POINTS) {
    pr[(size_t)row * AH_POINTS + tid] = s_pr[tid];
    pr_score[(size_t)row * AH_POINTS + tid] = s_sc[tid];
  }
}

extern "C" int fod_ap_hist_accum(const float* confs, const uint8_t* is_positive, const uint8_t* size_categories,
                                 const int64_t* num_annos, int T, int C1, long P_total, int* hist_tp, int* hist_seen,
                                 int64_t* anno_total, hipStream_t stream) {
  FOD_REQUIRE(T >= 1 && T <= AH_MAX_T, "ap_hist_accum: T=%d is outside 1..%d", T, AH_MAX_T);
  FOD_REQUIRE(C1 >= 2, "ap_hist_accum: C1=%d classes (the generic one included), at least 2 expected", C1);
  FOD_REQUIRE(P_total >= 1, "ap_hist_accum: P_total=%ld slots, at least 1 expected", P_total);
  const long nblk = (P_total + AH_THREADS - 1) / AH_THREADS;
  FOD_REQUIRE(nblk * C1 <= 0x7fffffffL, "ap_hist_accum: C1 * ceil(P_total / %d) = %ld workgroups", AH_THREADS, nblk * C1);
  FOD_REQUIRE(confs && is_positive && size_categories && num_annos && hist_tp && hist_seen && anno_total,
              "ap_hist_accum: null operand");
  hipLaunchKernelGGL(ap_hist_accum_kernel, dim3((unsigned)(nblk * C1)), dim3(AH_THREADS), 0, stream, confs, is_positive,
                     size_categories, (const long long*)num_annos, hist_tp, hist_seen, (unsigned long long*)anno_total, T,
                     C1, P_total, (int)nblk);
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}

extern "C" int fod_ap_hist_finalize(const int* hist_tp, const int* hist_seen, const int64_t* anno_total, int T, int C1,
                                    double* ap, double* ap101, double* pr, float* pr_score, int64_t* totals,
                                    hipStream_t stream) {
  FOD_REQUIRE(T >= 1 && T <= AH_MAX_T, "ap_hist_finalize: T=%d is outside 1..%d", T, AH_MAX_T);
  FOD_REQUIRE(C1 >= 2, "ap_hist_finalize: C1=%d classes (the generic one included), at least 2 expected", C1);
  FOD_REQUIRE((long)T * C1 * 4 <= 0x7fffffffL, "ap_hist_finalize: T * C1 * 4 = %ld workgroups", (long)T * C1 * 4);
  FOD_REQUIRE(hist_tp && hist_seen && anno_total && ap && ap101 && pr && pr_score && totals,
              "ap_hist_finalize: null operand");
  hipLaunchKernelGGL(ap_hist_finalize_kernel, dim3((unsigned)(T * C1 * 4)), dim3(AH_THREADS), 0, stream, hist_tp, hist_seen,
                     (const long long*)anno_total, ap, ap101, pr, pr_score, (long long*)totals, C1);
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}
