// What the kernels over DETECTION ROWS share (detect_nms.hip, detect_eval.hip, track.hip): the rows are the five tensors
// fod_detect_select writes -- scores f32 [B,K], labels i32 [B,K], boxes f32 [B,K,4] xyxy pixels, query i32 [B,K], count
// i32 [B] -- and every one of these kernels stages up to ROWS_MAX of them (or of annotations, or of track slots) in LDS.
#pragma once
#include "common.h"

// These kernels' tests (suppression, IoU, prediction, velocity) are defined in single roundings (include/fod_ext.h):
// nothing in a file that includes this header may contract a * b + c.  The arithmetic is written with plain operators
// for that reason: the pragma governs the operations written in the translation unit from here on, while __fmul_rn /
// __fsub_rn are inline functions of the HIP headers, compiled under the default (contracting) mode -- with them
// `(area_i + area_j) - iw * ih` came out as one v_fma_f32.  The pragma stands BEFORE the helpers below, and this header
// before any arithmetic of the including file: an expression above it would be contracted.
#pragma clang fp contract(off)

constexpr int ROWS_MAX = 1024;                         // = DET_MAX_K of fod_detect_select (csrc/loss.hip); also slots

// the rows of sample b that exist: rows at or beyond it are never read
FOD_DEVINL int row_count(const int32_t* count, int b, int K) { return min(max(count[b], 0), K); }

FOD_DEVINL bool row_finite(const float4 b) { return isfinite(b.x) && isfinite(b.y) && isfinite(b.z) && isfinite(b.w); }
FOD_DEVINL float4 row_box(const float* p) { return make_float4(p[0], p[1], p[2], p[3]); }     // (4-byte alignment only)
FOD_DEVINL void row_put(float* p, const float4 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }
FOD_DEVINL float row_area(const float4 b) { return fmaxf(b.z - b.x, 0.f) * fmaxf(b.w - b.y, 0.f); }   // clamped
FOD_DEVINL float row_inter(const float4 a, const float4 q) {
  return fmaxf(fminf(a.z, q.z) - fmaxf(a.x, q.x), 0.f) * fmaxf(fminf(a.w, q.w) - fmaxf(a.y, q.y), 0.f);
}

// a 64-bit word every lane holds alike, into scalar registers
FOD_DEVINL unsigned long long row_uniform64(unsigned long long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
// the value lane `i` holds, for a wave-uniform i: v_readlane_b32 into scalar registers, no LDS round trip
FOD_DEVINL int row_lane(int v, int i) { return __builtin_amdgcn_readlane(v, i); }
FOD_DEVINL float row_lane(float v, int i) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i)); }
FOD_DEVINL float4 row_lane(float4 v, int i) {
  return make_float4(row_lane(v.x, i), row_lane(v.y, i), row_lane(v.z, i), row_lane(v.w, i));
}
FOD_DEVINL unsigned long long row_lane(unsigned long long v, int i) {
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, i), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), i);
  return ((unsigned long long)hi << 32) | lo;
}
