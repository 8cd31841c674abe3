// Second launch of the deterministic (`_det`) entry points: the contributing workgroups of the first launch have written
// their partial results with plain stores into the caller's scratch; this kernel adds them up IN INDEX ORDER, one thread
// per output element, and stores (or adds to) the output once.  The sum depends on the launch geometry (how many
// partials there are), never on which workgroup finished first.  No tickets, no waiting: launches of one stream are
// ordered, so the partials are complete when this kernel starts.
#pragma once
#include "common.h"

namespace foddet {

// Batch z (blockIdx.y), partial s, element e:  part[z * part_batch + s * part_stride + e],  e in [0, n0 + n1).
// Elements [0, n0) go to out0 as an [n0 / cols0, cols0] matrix with row pitch ld0, elements [n0, n0 + n1) to out1.
// A partial whose element would lie at or past part_total (floats, within one batch) does not exist: the partials of
// an output row that fewer input rows map to (fod_mlp2_mul_bwd_det with M % table_rows != 0).
struct ReduceParams {
  const float* part;
  long part_stride, part_batch, part_total;
  int nparts;
  float* out0;
  int n0, cols0;
  long ld0, out0_batch;
  float* out1;
  int n1;
  long out1_batch;
  int accumulate;      // 1: out = old value + sum, 0: out = sum
};

}  // namespace foddet

namespace {

__global__ __launch_bounds__(256) void det_reduce_kernel(const foddet::ReduceParams p) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)p.n0 + p.n1) return;
  const float* src = p.part + (long)blockIdx.y * p.part_batch + e;
  int np = p.nparts;
  if (p.part_stride > 0) {
    const long fit = (p.part_total - e + p.part_stride - 1) / p.part_stride;      // partials that exist for this element
    if (fit < np) np = (int)(fit > 0 ? fit : 0);
  }
  float acc = 0.f;
  int s = 0;
  for (; s + 4 <= np; s += 4) {                     // four loads in flight, added in index order
    const float v0 = src[(s + 0) * p.part_stride];
    const float v1 = src[(s + 1) * p.part_stride];
    const float v2 = src[(s + 2) * p.part_stride];
    const float v3 = src[(s + 3) * p.part_stride];
    acc += v0;
    acc += v1;
    acc += v2;
    acc += v3;
  }
  for (; s < np; ++s) acc += src[s * p.part_stride];
  float* dst;
  if (e < p.n0) {
    const long i = e / p.cols0;
    dst = p.out0 + (long)blockIdx.y * p.out0_batch + i * p.ld0 + (e - i * p.cols0);
  } else {
    dst = p.out1 + (long)blockIdx.y * p.out1_batch + (e - p.n0);
  }
  *dst = p.accumulate ? *dst + acc : acc;
}

inline int det_reduce_launch(const foddet::ReduceParams& p, int batches, hipStream_t stream) {
  const long n = (long)p.n0 + p.n1;
  if (n <= 0 || batches <= 0) return FOD_OK;
  hipLaunchKernelGGL(det_reduce_kernel, dim3((unsigned)((n + 255) / 256), batches), dim3(256), 0, stream, p);
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}

// The scratch every deterministic entry point is handed: never optional, never replaced by atomics.
#define FOD_REQUIRE_SCRATCH(who, ws, ws_bytes, need)                                                              \
  FOD_REQUIRE((ws) != nullptr && ((uintptr_t)(ws) % 16) == 0 && (size_t)(ws_bytes) >= (size_t)(need),             \
              "%s: scratch missing or too small (ws %p, %zu bytes, %zu needed): the deterministic form has no " \
              "atomic fallback", who, (const void*)(ws), (size_t)(ws_bytes), (size_t)(need))

}  // namespace
