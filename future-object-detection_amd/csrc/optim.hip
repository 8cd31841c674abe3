// Global-norm gradient clipping + AdamW over MANY parameter tensors in two launches (a table of
// pointers instead of one launch per tensor): torch.optim.AdamW / clip_grad_norm_ semantics, reference
// future_od/trainer.py:186-188 and runs/_helper.py:84-107.  HBM-bound: reads p, g, m, v once, writes
// p, m, v once.  Every tensor is processed as its dense storage order, so parameter, gradient and both
// moments must share one memory layout (the host wrapper checks).
// Behind them: the exponential moving average of the weights, its in-place swap and the gradient accumulation between
// the replays of a captured backward (include/fod_ext.h), same geometry.
#include "common.h"

#include "../../include/fod_ext.h"

namespace {

constexpr int CHUNK = 16384;   // elements per block (16 float4 per thread: ~3300 blocks for the 54 M parameters)

struct Slot {
  long n;
  float* p;
  const float* g;
  float* m;
  float* v;
  float lr, wd;
};

__global__ __launch_bounds__(256) void multi_sqnorm_kernel(const long* __restrict__ ptrs, const long* __restrict__ numel,
                                                           const int* __restrict__ blk_tensor,
                                                           const int* __restrict__ blk_chunk, float* __restrict__ out) {
  __shared__ float red[4];
  const int t = blk_tensor[blockIdx.x];
  const long base = (long)blk_chunk[blockIdx.x] * CHUNK;
  const long end = min(numel[t], base + CHUNK);
  const float* g = reinterpret_cast<const float*>(ptrs[t * 4 + 1]);
  float s = 0.f;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {          // 16 bytes per lane (CHUNK is a multiple of 4)
    const long end4 = base + ((end - base) & ~3L);
    // all of the thread's loads of the chunk in flight at once; summed in the same order as a rolled loop would
    constexpr int NIT = CHUNK / 1024;
    float4 q[NIT];
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
      const long i = base + 4 * threadIdx.x + 1024L * k;
      q[k] = i < end4 ? *reinterpret_cast<const float4*>(g + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
      const long i = base + 4 * threadIdx.x + 1024L * k;
      if (i < end4) s += q[k].x * q[k].x + q[k].y * q[k].y + q[k].z * q[k].z + q[k].w * q[k].w;
    }
    for (long i = end4 + threadIdx.x; i < end; i += 256) s += g[i] * g[i];
  } else {
    for (long i = base + threadIdx.x; i < end; i += 256) s += g[i] * g[i];
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

// The same sum with a FIXED summation order: every block stores its partial, takes a ticket, and the block that draws
// the last ticket adds the partials in index order (no spinning: nobody waits for anybody).  Data-parallel ranks that
// hold equal gradients then compute bit-equal norms -- with the atomic form above the clip factor differs in its last
// bit from rank to rank and the replicas drift apart (tests/test_parallel_gpu.py measured 1 ulp after 7 steps).
__global__ __launch_bounds__(256) void multi_sqnorm_det_kernel(const long* __restrict__ ptrs, const long* __restrict__ numel,
                                                               const int* __restrict__ blk_tensor,
                                                               const int* __restrict__ blk_chunk, float* __restrict__ out,
                                                               float* __restrict__ partial, unsigned* __restrict__ ticket) {
  __shared__ float red[4];
  __shared__ bool last;
  const int t = blk_tensor[blockIdx.x];
  const long base = (long)blk_chunk[blockIdx.x] * CHUNK;
  const long end = min(numel[t], base + CHUNK);
  const float* g = reinterpret_cast<const float*>(ptrs[t * 4 + 1]);
  float s = 0.f;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    const long end4 = base + ((end - base) & ~3L);
    // all of the thread's loads of the chunk in flight at once; summed in the same order as a rolled loop would
    constexpr int NIT = CHUNK / 1024;
    float4 q[NIT];
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
      const long i = base + 4 * threadIdx.x + 1024L * k;
      q[k] = i < end4 ? *reinterpret_cast<const float4*>(g + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
      const long i = base + 4 * threadIdx.x + 1024L * k;
      if (i < end4) s += q[k].x * q[k].x + q[k].y * q[k].y + q[k].z * q[k].z + q[k].w * q[k].w;
    }
    for (long i = end4 + threadIdx.x; i < end; i += 256) s += g[i] * g[i];
  } else {
    for (long i = base + threadIdx.x; i < end; i += 256) s += g[i] * g[i];
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    store_sc1(partial + blockIdx.x, (red[0] + red[1]) + (red[2] + red[3]));
    stores_done();                                     // sc1 hand-off (common.h): no fences
    last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  }
  __syncthreads();                                     // the other waves load after the barrier the adding wave joins
  if (!last) return;
  float a = 0.f;
  for (unsigned i = threadIdx.x; i < gridDim.x; i += 256) a += load_sc1(partial + i);
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = (red[0] + red[1]) + (red[2] + red[3]);
    *ticket = 0u;                                      // ready for the next launch (stream-ordered)
  }
}

__global__ __launch_bounds__(256) void multi_adamw_kernel(const long* __restrict__ ptrs, const long* __restrict__ numel,
                                                          const float* __restrict__ lr_wd,
                                                          const int* __restrict__ blk_tensor,
                                                          const int* __restrict__ blk_chunk, float b1, float b2,
                                                          float eps, float bc1, float bc2,
                                                          const float* __restrict__ bias_dev,
                                                          const float* __restrict__ sqnorm, float max_norm) {
  if (bias_dev) {            // bias corrections kept on the device (captured steps: the step count lives there)
    bc1 = bias_dev[0];
    bc2 = bias_dev[1];
  }
  const int t = blk_tensor[blockIdx.x];
  const long base = (long)blk_chunk[blockIdx.x] * CHUNK;
  const long end = min(numel[t], base + CHUNK);
  float* p = reinterpret_cast<float*>(ptrs[t * 4 + 0]);
  const float* g = reinterpret_cast<const float*>(ptrs[t * 4 + 1]);
  float* m = reinterpret_cast<float*>(ptrs[t * 4 + 2]);
  float* v = reinterpret_cast<float*>(ptrs[t * 4 + 3]);
  const float lr = lr_wd[t * 2], wd = lr_wd[t * 2 + 1];
  float cs = 1.f;
  if (max_norm > 0.f && sqnorm) cs = fminf(1.f, max_norm / (sqrtf(*sqnorm) + 1e-6f));   // clip_grad_norm_
  const float step = lr / bc1, rs2 = 1.f / sqrtf(bc2);
  auto update = [&](float& pp, float gg, float& mm, float& vv_) {
    const float gr = gg * cs;
    const float mv = b1 * mm + (1.f - b1) * gr;
    const float vv = b2 * vv_ + (1.f - b2) * gr * gr;
    mm = mv;
    vv_ = vv;
    pp = pp * (1.f - lr * wd) - step * (mv / (sqrtf(vv) * rs2 + eps));
  };
  long tail = base;
  if (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
        reinterpret_cast<uintptr_t>(v)) & 15) == 0) {          // 16 bytes per lane and stream (HBM-bound: 28 B / element)
    const long end4 = base + ((end - base) & ~3L);
    for (long i = base + 4 * threadIdx.x; i < end4; i += 1024) {
      float4 pq = *reinterpret_cast<float4*>(p + i), mq = *reinterpret_cast<float4*>(m + i),
             vq = *reinterpret_cast<float4*>(v + i);
      const float4 gq = *reinterpret_cast<const float4*>(g + i);
      update(pq.x, gq.x, mq.x, vq.x);
      update(pq.y, gq.y, mq.y, vq.y);
      update(pq.z, gq.z, mq.z, vq.z);
      update(pq.w, gq.w, mq.w, vq.w);
      *reinterpret_cast<float4*>(m + i) = mq;
      *reinterpret_cast<float4*>(v + i) = vq;
      *reinterpret_cast<float4*>(p + i) = pq;
    }
    tail = end4;
  }
  for (long i = tail + threadIdx.x; i < end; i += 256) update(p[i], g[i], m[i], v[i]);
}

// Exponential moving average of the weights over MANY tensors in one launch (include/fod_ext.h): the geometry of
// multi_adamw_kernel -- the same CHUNK, the same block tables -- over (average, parameter) pairs.  HBM-bound at
// 12 B / element: reads e and p, writes e.  The number of the update is read from device memory and every block forms
// the weight itself, so a captured launch bakes in no host scalar that changes from step to step.
FOD_DEVINL float ema_weight(long long u, float decay, int warmup) {
  double d = (double)decay;
  if (warmup) d = fmin(d, (1.0 + (double)u) / (10.0 + (double)u));
  return (float)(1.0 - d);
}

// e + w * (p - e), each of the three operations rounded on its own: the float32 restatement in numpy gives the same
// bits.  The pragma is what keeps the product and the sum apart -- __fmul_rn / __fadd_rn are plain operators in
// inline functions here, and hipcc's default contraction fused them into v_pk_fma_f32 / v_fmac_f32 all the same.
FOD_DEVINL float ema_step(float e, float p, float w) {
#pragma clang fp contract(off)
  const float diff = p - e;
  const float move = w * diff;
  return e + move;
}

__global__ __launch_bounds__(256) void multi_ema_kernel(const long* __restrict__ pairs, const long* __restrict__ numel,
                                                        const int* __restrict__ blk_tensor,
                                                        const int* __restrict__ blk_chunk,
                                                        const long long* __restrict__ updates, float decay, int warmup) {
  const float w = ema_weight(*updates, decay, warmup);
  const int t = blk_tensor[blockIdx.x];
  const long base = (long)blk_chunk[blockIdx.x] * CHUNK;
  const long end = min(numel[t], base + CHUNK);
  float* e = reinterpret_cast<float*>(pairs[t * 2 + 0]);
  const float* p = reinterpret_cast<const float*>(pairs[t * 2 + 1]);
  long tail = base;
  if (((reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(p)) & 15) == 0) {      // 16 bytes per lane and stream
    const long end4 = base + ((end - base) & ~3L);
    for (long i = base + 4 * threadIdx.x; i < end4; i += 1024) {
      float4 eq = *reinterpret_cast<float4*>(e + i);
      const float4 pq = *reinterpret_cast<const float4*>(p + i);
      eq.x = ema_step(eq.x, pq.x, w);
      eq.y = ema_step(eq.y, pq.y, w);
      eq.z = ema_step(eq.z, pq.z, w);
      eq.w = ema_step(eq.w, pq.w, w);
      *reinterpret_cast<float4*>(e + i) = eq;
    }
    tail = end4;
  }
  for (long i = tail + threadIdx.x; i < end; i += 256) e[i] = ema_step(e[i], p[i], w);
}

// The two tensors of every pair change contents, bit for bit (words are moved, never interpreted).
__global__ __launch_bounds__(256) void multi_swap_kernel(const long* __restrict__ pairs, const long* __restrict__ numel,
                                                         const int* __restrict__ blk_tensor,
                                                         const int* __restrict__ blk_chunk) {
  const int t = blk_tensor[blockIdx.x];
  const long base = (long)blk_chunk[blockIdx.x] * CHUNK;
  const long end = min(numel[t], base + CHUNK);
  unsigned* a = reinterpret_cast<unsigned*>(pairs[t * 2 + 0]);
  unsigned* b = reinterpret_cast<unsigned*>(pairs[t * 2 + 1]);
  long tail = base;
  if (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0) {
    const long end4 = base + ((end - base) & ~3L);
    for (long i = base + 4 * threadIdx.x; i < end4; i += 1024) {
      const uint4 aq = *reinterpret_cast<const uint4*>(a + i), bq = *reinterpret_cast<const uint4*>(b + i);
      *reinterpret_cast<uint4*>(a + i) = bq;
      *reinterpret_cast<uint4*>(b + i) = aq;
    }
    tail = end4;
  }
  for (long i = tail + threadIdx.x; i < end; i += 256) {
    const unsigned av = a[i], bv = b[i];
    a[i] = bv;
    b[i] = av;
  }
}

// Gradient accumulation between replays of a captured backward (include/fod_ext.h): the geometry of multi_ema_kernel
// over (accumulator, gradient) pairs.  MODE 0 moves words (acc = g, 8 B / element), MODE 1 adds (acc = acc + g,
// 12 B / element), MODE 2 finishes (g = (acc + g) * scale, 12 B / element).  Every element is written by exactly one
// thread, no atomics: the result does not depend on timing, which is what deterministic mode needs of it.
FOD_DEVINL float accum_add(float a, float g) {
#pragma clang fp contract(off)
  return a + g;
}

// the sum and the product each rounded on their own, as ema_step does it
FOD_DEVINL float accum_finish(float a, float g, float scale) {
#pragma clang fp contract(off)
  const float sum = a + g;
  return sum * scale;
}

template <int MODE>
__global__ __launch_bounds__(256) void multi_accum_kernel(const long* __restrict__ pairs, const long* __restrict__ numel,
                                                          const int* __restrict__ blk_tensor,
                                                          const int* __restrict__ blk_chunk, float scale) {
  const int t = blk_tensor[blockIdx.x];
  const long base = (long)blk_chunk[blockIdx.x] * CHUNK;
  const long end = min(numel[t], base + CHUNK);
  float* a = reinterpret_cast<float*>(pairs[t * 2 + 0]);
  float* g = reinterpret_cast<float*>(pairs[t * 2 + 1]);
  long tail = base;
  if (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(g)) & 15) == 0) {      // 16 bytes per lane and stream
    const long end4 = base + ((end - base) & ~3L);
    for (long i = base + 4 * threadIdx.x; i < end4; i += 1024) {
      if (MODE == 0) {
        *reinterpret_cast<uint4*>(a + i) = *reinterpret_cast<const uint4*>(g + i);
      } else {
        float4 aq = *reinterpret_cast<const float4*>(a + i);
        const float4 gq = *reinterpret_cast<const float4*>(g + i);
        if (MODE == 1) {
          aq.x = accum_add(aq.x, gq.x);
          aq.y = accum_add(aq.y, gq.y);
          aq.z = accum_add(aq.z, gq.z);
          aq.w = accum_add(aq.w, gq.w);
          *reinterpret_cast<float4*>(a + i) = aq;
        } else {
          aq.x = accum_finish(aq.x, gq.x, scale);
          aq.y = accum_finish(aq.y, gq.y, scale);
          aq.z = accum_finish(aq.z, gq.z, scale);
          aq.w = accum_finish(aq.w, gq.w, scale);
          *reinterpret_cast<float4*>(g + i) = aq;
        }
      }
    }
    tail = end4;
  }
  for (long i = tail + threadIdx.x; i < end; i += 256) {
    if (MODE == 0)
      reinterpret_cast<unsigned*>(a)[i] = reinterpret_cast<const unsigned*>(g)[i];
    else if (MODE == 1)
      a[i] = accum_add(a[i], g[i]);
    else
      g[i] = accum_finish(a[i], g[i], scale);
  }
}

}  // namespace

extern "C" int fod_multi_sqnorm_acc(const long* ptrs, const long* numel, const int* blk_tensor, const int* blk_chunk,
                                    int nblocks, float* out, hipStream_t stream) {
  FOD_REQUIRE(ptrs && numel && blk_tensor && blk_chunk && out && nblocks > 0, "multi_sqnorm: bad args");
  hipLaunchKernelGGL(multi_sqnorm_kernel, dim3(nblocks), dim3(256), 0, stream, ptrs, numel, blk_tensor, blk_chunk, out);
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}

extern "C" int fod_multi_sqnorm_det(const long* ptrs, const long* numel, const int* blk_tensor, const int* blk_chunk,
                                    int nblocks, float* out, float* scratch, hipStream_t stream) {
  FOD_REQUIRE(ptrs && numel && blk_tensor && blk_chunk && out && scratch && nblocks > 0, "multi_sqnorm_det: bad args");
  hipLaunchKernelGGL(multi_sqnorm_det_kernel, dim3(nblocks), dim3(256), 0, stream, ptrs, numel, blk_tensor, blk_chunk, out,
                     scratch + 1, reinterpret_cast<unsigned*>(scratch));
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}

extern "C" int fod_multi_adamw(const long* ptrs, const long* numel, const float* lr_wd, const int* blk_tensor,
                               const int* blk_chunk, int nblocks, float beta1, float beta2, float eps, float bias_c1,
                               float bias_c2, const float* bias_dev, const float* sqnorm, float max_norm,
                               hipStream_t stream) {
  FOD_REQUIRE(ptrs && numel && lr_wd && blk_tensor && blk_chunk && nblocks > 0, "multi_adamw: bad args");
  hipLaunchKernelGGL(multi_adamw_kernel, dim3(nblocks), dim3(256), 0, stream, ptrs, numel, lr_wd, blk_tensor,
                     blk_chunk, beta1, beta2, eps, bias_c1, bias_c2, bias_dev, sqnorm, max_norm);
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}

extern "C" int fod_multi_chunk(void) { return CHUNK; }

extern "C" int fod_multi_ema(const long* pairs, const long* numel, const int* blk_tensor, const int* blk_chunk,
                             int nblocks, const long long* updates_dev, float decay, int warmup, hipStream_t stream) {
  FOD_REQUIRE(pairs && numel && blk_tensor && blk_chunk && updates_dev && nblocks > 0, "multi_ema: bad args");
  FOD_REQUIRE(decay >= 0.f && decay <= 1.f, "multi_ema: decay %g is not in [0, 1]", (double)decay);
  hipLaunchKernelGGL(multi_ema_kernel, dim3(nblocks), dim3(256), 0, stream, pairs, numel, blk_tensor, blk_chunk,
                     updates_dev, decay, warmup);
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}

extern "C" int fod_multi_swap(const long* pairs, const long* numel, const int* blk_tensor, const int* blk_chunk,
                              int nblocks, hipStream_t stream) {
  FOD_REQUIRE(pairs && numel && blk_tensor && blk_chunk && nblocks > 0, "multi_swap: bad args");
  hipLaunchKernelGGL(multi_swap_kernel, dim3(nblocks), dim3(256), 0, stream, pairs, numel, blk_tensor, blk_chunk);
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}

extern "C" int fod_multi_accum(const long* pairs, const long* numel, const int* blk_tensor, const int* blk_chunk,
                               int nblocks, int mode, float scale, hipStream_t stream) {
  FOD_REQUIRE(pairs && numel && blk_tensor && blk_chunk && nblocks > 0, "multi_accum: bad args");
  FOD_REQUIRE(mode >= 0 && mode <= 2, "multi_accum: mode %d is not 0 (store), 1 (add) or 2 (finish)", mode);
  FOD_REQUIRE(scale > 0.f && scale <= 3.402823466e38f, "multi_accum: scale %g is not finite and > 0", (double)scale);
  if (mode == 0)
    hipLaunchKernelGGL(multi_accum_kernel<0>, dim3(nblocks), dim3(256), 0, stream, pairs, numel, blk_tensor, blk_chunk,
                       scale);
  else if (mode == 1)
    hipLaunchKernelGGL(multi_accum_kernel<1>, dim3(nblocks), dim3(256), 0, stream, pairs, numel, blk_tensor, blk_chunk,
                       scale);
  else
    hipLaunchKernelGGL(multi_accum_kernel<2>, dim3(nblocks), dim3(256), 0, stream, pairs, numel, blk_tensor, blk_chunk,
                       scale);
  FOD_LAUNCH_CHECK();
  return FOD_OK;
}
