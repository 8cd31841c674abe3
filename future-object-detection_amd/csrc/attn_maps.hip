// Attention maps for looking at a trained model (reference demo.ipynb: SlotToImageAttention.store_attention and the
// head mean of the softmax weights): the head-averaged cross-attention of SELECTED queries over the keys of up to 32
// memory images, in ONE launch.  include/fod_ext.h (fod_attn_maps) states the map.
//
//   out[b, i, j, s] = (1/H) sum_h softmax_s((q1_h . k1_h + q2_h . k2_h) * scale)     query query_idx[b, i], image j
//
// The work is small (B = 2, J = 5, Q = 100, S = 1450, H = 8: 1.5 GFLOP a pass) and bound by latency and key bytes, not
// by the matrix pipe.  A 32-query accumulator over all keys of all heads does not fit the LDS, so a workgroup makes
// two passes over the keys:
//   (a) per head, the running maximum and sum of exp2 over ALL keys -> (max2, log2 sum) [h][q] in LDS; a wave owns the
//       heads h = wave, wave + 8, ..., so the eight waves never meet before the barrier;
//   (b) per 32-key tile of the workgroup's key chunk, the scores of every head are recomputed, exp2(x - max2 - log2 sum)
//       is added up over the heads and the tile is stored once, times 1/H; a wave owns the tiles wave, wave + 8, ...
// The score tile is queries x keys with the KEY on the lane (C/D layout of the 32x32 MFMA, common.h): the statistics
// of pass (a) stay per lane until one shuffle reduction per head, and the stores of pass (b) are 128-byte rows.
// Grid: (query tile x key chunk, image, batch element).  32 queries is the MFMA's tile; so that a launch with few
// queries still fills the chip (Q = 100, J = 5, B = 2: 40 query tiles on 256 CUs) the keys of pass (b) are cut into up
// to 8 chunks of at least 256 keys (a tile per wave), one workgroup each.  Every chunk's workgroup repeats pass (a) in
// full: nothing is handed from block to block, every output element has exactly one writer, there are no atomics --
// the result does not depend on timing.
// bf16 operands: v_mfma_f32_32x32x16_bf16, products exact, sums in f32.  f32 operands: v_mfma_f32_32x32x2_f32, an f32
// fma chain on the unrounded operands.
#include "common.h"
#include "../../include/fod_ext.h"

namespace {

// 2^x as one v_exp_f32 (attention.hip: ex2): every argument here is <= 0 up to rounding
FOD_DEVINL float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

constexpr float LOG2E = 1.4426950408889634f;
constexpr int AM_MAX_JOBS = 32;
constexpr int AM_MAX_H = 64;                 // the statistics of pass (a): 2 x 64 x 32 f32 = 16 KiB of LDS
constexpr int AM_MAX_Q = 1024;               // the matcher's query limit
constexpr int AM_MAX_SPLIT = 8;
constexpr int AM_WAVES = 8, AM_THREADS = 64 * AM_WAVES;

struct MapJob {
  const void *q1, *q2, *k1, *k2;
};
struct MapJobs {
  MapJob j[AM_MAX_JOBS];
};
struct MapParams {
  int B, H, Tq, S, Q, njobs;
  int ksplit, kchunk;                        // key chunks of pass (b): kchunk is a multiple of 32
  long q_bs, q_ts, k_bs, k_ts, k2_bs, k2_ts;
  float c;                                   // scale * log2(e)
  float inv_h;
  const int* query_idx;
  float* out;
};

// the four operand fragments of one 32-row tile and one head: [part][k-step of 16 channels]
template <typename T, int PARTS>
struct Rows {
  Frag<T> f[PARTS][2];
};

template <typename T, int PARTS>
FOD_DEVINL void load_rows(Rows<T, PARTS>& x, const T* p1, const T* p2) {
  frag_load_contig(x.f[0][0], p1);
  frag_load_contig(x.f[0][1], p1 + 16);
  if (PARTS == 2) {
    frag_load_contig(x.f[PARTS - 1][0], p2);
    frag_load_contig(x.f[PARTS - 1][1], p2 + 16);
  }
}

template <typename T, int PARTS>
FOD_DEVINL f32x16 scores(const Rows<T, PARTS>& q, const Rows<T, PARTS>& k) {
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int part = 0; part < PARTS; ++part) {
    mma16(q.f[part][0], k.f[part][0], acc);
    mma16(q.f[part][1], k.f[part][1], acc);
  }
  return acc;
}

// pass (a), one 32-key tile: the tile's scores join the running maximum m and sum l of the lane's key class
template <typename T, int PARTS>
FOD_DEVINL void fold_tile(const Rows<T, PARTS>& q, const Rows<T, PARTS>& k, bool k_ok, float c, float (&m)[16],
                          float (&l)[16]) {
  const f32x16 acc = scores<T, PARTS>(q, k);
  float x[16];
  bool grows = false;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    x[g] = acc[g] * c;
    grows |= k_ok && x[g] > m[g];
  }
  if (__any(grows)) {                                          // rare after the first tiles: the rescale is skipped
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const float mn = k_ok ? fmaxf(m[g], x[g]) : m[g];
      l[g] = mn == m[g] ? l[g] : l[g] * ex2(m[g] - mn);        // (m = -inf: l is 0, and ex2(-inf) = 0)
      m[g] = mn;
    }
  }
#pragma unroll
  for (int g = 0; g < 16; ++g) l[g] += k_ok ? ex2(x[g] - m[g]) : 0.f;
}

// pass (b), one head of one tile: the head's probabilities join the sum over the heads
template <typename T, int PARTS>
FOD_DEVINL void add_head(const Rows<T, PARTS>& q, const Rows<T, PARTS>& k, const float* s_max_h, const float* s_lsum_h,
                         int hh, float c, float (&prob)[16]) {
  const f32x16 acc = scores<T, PARTS>(q, k);
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    const f32x4 mx = *reinterpret_cast<const f32x4*>(s_max_h + 8 * g4 + 4 * hh);
    const f32x4 ls = *reinterpret_cast<const f32x4*>(s_lsum_h + 8 * g4 + 4 * hh);
#pragma unroll
    for (int e = 0; e < 4; ++e) prob[4 * g4 + e] += ex2((acc[4 * g4 + e] * c - mx[e]) - ls[e]);
  }
}

template <typename T, int PARTS>
__global__ __launch_bounds__(AM_THREADS) void attn_maps_kernel(const MapParams p, const MapJobs jobs) {
  __shared__ __attribute__((aligned(16))) float s_max[AM_MAX_H][32];      // max2 of head h, query row
  __shared__ __attribute__((aligned(16))) float s_lsum[AM_MAX_H][32];     // log2 of the sum of exp2(x - max2)
  constexpr int U = sizeof(T) == 2 ? 2 : 1;  // key tiles per load group of pass (a); two groups are in flight
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int qtile = blockIdx.x / p.ksplit, split = blockIdx.x - qtile * p.ksplit;
  const int job = blockIdx.y, b = blockIdx.z;
  const int q0 = qtile * 32;
  const MapJob& jb = jobs.j[job];

  // the lane's query row: an index outside [0, Tq) reads row 0 and is written as zeros
  const int i = q0 + r;
  int qi = -1;
  if (i < p.Q) qi = p.query_idx ? p.query_idx[(long)b * p.Q + i] : i;
  const bool q_ok = qi >= 0 && qi < p.Tq;
  const unsigned row_ok = (unsigned)__ballot(q_ok);           // bit = query row of the tile (both lane halves agree)
  const long q_off = (long)b * p.q_bs + (long)(q_ok ? qi : 0) * p.q_ts + 8 * hh;
  const T* q1 = (const T*)jb.q1 + q_off;
  const T* q2 = PARTS == 2 ? (const T*)jb.q2 + q_off : nullptr;
  const T* k1 = (const T*)jb.k1 + (long)b * p.k_bs + 8 * hh;
  const T* k2 = PARTS == 2 ? (const T*)jb.k2 + (long)b * p.k2_bs + 8 * hh : nullptr;
  const int ntiles = (p.S + 31) / 32;

  // ---- (a) per head: maximum and sum over all keys.  The loads of the next group of tiles are issued before the
  // current group is folded in (two register buffers, the loop body holds both so that neither is indexed).
  for (int h = wave; h < p.H; h += AM_WAVES) {
    Rows<T, PARTS> q;
    load_rows<T, PARTS>(q, q1 + 32 * h, q2 + 32 * h);
    float m[16], l[16];
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      m[g] = -INFINITY;
      l[g] = 0.f;
    }
    Rows<T, PARTS> ka[U], kb[U];
    auto load_group = [&](Rows<T, PARTS>(&k)[U], int t0) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long key = min((t0 + u) * 32 + r, p.S - 1);      // past the end: the last row again, masked in fold_tile
        load_rows<T, PARTS>(k[u], k1 + key * p.k_ts + 32 * h, k2 + key * p.k2_ts + 32 * h);
      }
    };
    auto fold_group = [&](const Rows<T, PARTS>(&k)[U], int t0) {
#pragma unroll
      for (int u = 0; u < U; ++u) fold_tile<T, PARTS>(q, k[u], (t0 + u) * 32 + r < p.S, p.c, m, l);
    };
    load_group(ka, 0);
    for (int t0 = 0; t0 < ntiles; t0 += 2 * U) {
      load_group(kb, t0 + U);
      fold_group(ka, t0);
      load_group(ka, t0 + 2 * U);
      if (t0 + U < ntiles) fold_group(kb, t0 + U);
    }
    // the 32 lanes of a half hold 32 key classes of the same 16 query rows
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      float mx = m[g];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
      float sum = m[g] == -INFINITY ? 0.f : l[g] * ex2(m[g] - mx);
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
      if (r == 0) {
        s_max[h][acc_row(g, lane)] = mx;
        s_lsum[h][acc_row(g, lane)] = log2f(sum);
      }
    }
  }
  __syncthreads();

  // ---- (b) the tiles of this workgroup's key chunk; the operands of head h + 1 are loaded before head h is added up
  const int t_begin = split * (p.kchunk / 32), t_end = min(t_begin + p.kchunk / 32, ntiles);
  for (int t = t_begin + wave; t < t_end; t += AM_WAVES) {
    const int key_lane = t * 32 + r;
    const long key = min(key_lane, p.S - 1);
    const T* kr1 = k1 + key * p.k_ts;
    const T* kr2 = PARTS == 2 ? k2 + key * p.k2_ts : nullptr;
    float prob[16];
#pragma unroll
    for (int g = 0; g < 16; ++g) prob[g] = 0.f;
    Rows<T, PARTS> qa, ka, qb, kb;
    auto load_head = [&](Rows<T, PARTS>& q, Rows<T, PARTS>& k, int h) {
      load_rows<T, PARTS>(k, kr1 + 32 * h, kr2 + 32 * h);
      load_rows<T, PARTS>(q, q1 + 32 * h, q2 + 32 * h);       // (the same 32 rows for every tile: cache hits)
    };
    load_head(qa, ka, 0);
    for (int h = 0; h < p.H; h += 2) {
      if (h + 1 < p.H) load_head(qb, kb, h + 1);               // (a head past the last one would leave the row)
      add_head<T, PARTS>(qa, ka, s_max[h], s_lsum[h], hh, p.c, prob);
      if (h + 2 < p.H) load_head(qa, ka, h + 2);
      if (h + 1 < p.H) add_head<T, PARTS>(qb, kb, s_max[h + 1], s_lsum[h + 1], hh, p.c, prob);
    }
    if (key_lane < p.S) {
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int row = acc_row(g, lane);
        if (q0 + row < p.Q)
          p.out[(((long)b * p.Q + q0 + row) * p.njobs + job) * p.S + key_lane] =
              (row_ok >> row & 1u) ? prob[g] * p.inv_h : 0.f;
      }
    }
  }
}

}  // namespace

extern "C" int fod_attn_maps(int dtype, int njobs, const void* const* ptrs, const int* query_idx, int Q, float* out,
                             const fod_attn_shape* s, hipStream_t stream) {
  FOD_REQUIRE(dtype == FOD_BF16 || dtype == FOD_F32, "attn_maps: bad dtype %d", dtype);
  FOD_REQUIRE(ptrs && njobs >= 1 && njobs <= AM_MAX_JOBS, "attn_maps: 1 .. %d jobs (%d)", AM_MAX_JOBS, njobs);
  FOD_REQUIRE(s, "attn_maps: null shape");
  FOD_REQUIRE(Q >= 1 && Q <= AM_MAX_Q, "attn_maps: %d selected queries, not 1..%d", Q, AM_MAX_Q);
  FOD_REQUIRE(s->Tq >= 1 && s->Tq <= AM_MAX_Q, "attn_maps: Tq %d, not 1..%d", s->Tq, AM_MAX_Q);
  FOD_REQUIRE(s->S >= 1, "attn_maps: S %d is below 1", s->S);
  FOD_REQUIRE(s->B >= 1 && s->B <= 65535 && s->H >= 1 && s->H <= AM_MAX_H, "attn_maps: bad extent B %d, H %d (H <= %d)",
              s->B, s->H, AM_MAX_H);
  FOD_REQUIRE(query_idx || Q == s->Tq, "attn_maps: without query_idx Q (%d) must equal Tq (%d)", Q, s->Tq);
  FOD_REQUIRE(out, "attn_maps: null out");
  FOD_REQUIRE(s->drop_p == 0.f, "attn_maps: drop_p = %f; the map is the probabilities before dropout", s->drop_p);
  FOD_REQUIRE((long)s->B * Q * njobs * s->S < (1L << 40), "attn_maps: output too large");
  MapParams p{};
  p.B = s->B; p.H = s->H; p.Tq = s->Tq; p.S = s->S; p.Q = Q; p.njobs = njobs;
  p.q_bs = s->q_batch_stride; p.q_ts = s->q_token_stride;
  p.k_bs = s->k_batch_stride; p.k_ts = s->k_token_stride;
  const bool own2 = s->k2_token_stride != 0;                   // as fod_attn_fwd: 0 = the strides of k1
  p.k2_bs = own2 ? s->k2_batch_stride : p.k_bs;
  p.k2_ts = own2 ? s->k2_token_stride : p.k_ts;
  FOD_REQUIRE(p.q_ts % 8 == 0 && p.k_ts % 8 == 0 && p.q_bs % 8 == 0 && p.k_bs % 8 == 0 && p.k2_bs % 8 == 0 &&
                  p.k2_ts % 8 == 0, "attn_maps: strides must be multiples of 8 elements");
  FOD_REQUIRE(p.q_ts >= 0 && p.k_ts >= 0 && p.q_bs >= 0 && p.k_bs >= 0 && p.k2_bs >= 0 && p.k2_ts >= 0,
              "attn_maps: negative stride");
  p.c = s->scale * LOG2E;
  p.inv_h = 1.f / (float)s->H;
  p.query_idx = query_idx;
  p.out = out;
  MapJobs jobs{};
  bool parts2 = false;
  for (int i = 0; i < njobs; ++i) {
    const void* const* q = ptrs + 4 * i;
    MapJob& j = jobs.j[i];
    j.q1 = q[0]; j.q2 = q[1]; j.k1 = q[2]; j.k2 = q[3];
    FOD_REQUIRE(j.q1 && j.k1, "attn_maps: null operand in job %d", i);
    const bool two = j.q2 != nullptr;
    FOD_REQUIRE(two == (j.k2 != nullptr), "attn_maps: q2 / k2 of job %d must come together", i);
    FOD_REQUIRE(i == 0 || two == parts2, "attn_maps: jobs with and without a second part in one launch");
    FOD_REQUIRE((((uintptr_t)j.q1 | (uintptr_t)j.q2 | (uintptr_t)j.k1 | (uintptr_t)j.k2) & 15u) == 0,
                "attn_maps: operands of job %d are not 16-byte aligned", i);
    parts2 = two;
  }
  // key chunks of pass (b): as many as fill the chip, each at least 256 keys (one tile per wave), at most 8
  const long tiles = (long)ceil_div(Q, 32) * njobs * p.B;
  int ks = (int)(256 / tiles);
  ks = ks > AM_MAX_SPLIT ? AM_MAX_SPLIT : ks;
  ks = ks > p.S / (32 * AM_WAVES) ? p.S / (32 * AM_WAVES) : ks;
  ks = ks < 1 ? 1 : ks;
  p.kchunk = ceil_div(ceil_div(p.S, ks), 32) * 32;
  p.ksplit = ceil_div(p.S, p.kchunk);
  const dim3 grid(ceil_div(Q, 32) * p.ksplit, njobs, p.B), block(AM_THREADS);
  if (dtype == FOD_BF16) {
    if (parts2) hipLaunchKernelGGL((attn_maps_kernel<__bf16, 2>), grid, block, 0, stream, p, jobs);
    else hipLaunchKernelGGL((attn_maps_kernel<__bf16, 1>), grid, block, 0, stream, p, jobs);
  } else {
    if (parts2) hipLaunchKernelGGL((attn_maps_kernel<float, 2>), grid, block, 0, stream, p, jobs);
    else hipLaunchKernelGGL((attn_maps_kernel<float, 1>), grid, block, 0, stream, p, jobs);
  }
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}
