// Shared between gemm_tn.hip (128 x 128 tiles, register-staged ring) and gemm_tn_big.hip (8-wave tiles, LDS-DMA ring).
#pragma once
#include "common.h"
#include "knobs.h"

namespace fodtn {

enum { MODE_DENSE = 0, MODE_CONV = 1 };

struct TnParams {
  const void* G;
  const void* X;
  float* dW;
  long ldg, ldx, ldw;
  int M, N1, K2;
  const float* rscale;
  float* colsum;     // optional f32 [N1]: += column sums of G (bias gradient), done by the blockIdx.x == 0 blocks
  int accumulate;    // 0: outputs are all-zero on entry (caller's guarantee) -> a single M-split may plain-store
  int m_per_split;
  int tj, ti, nsplit, xcd_order;   // tile grid, number of M-splits, 1 = XCD-grouped 1-D launch
  unsigned g_bytes, x_bytes;       // operand extents for the buffer descriptors (< 4 GiB, host-checked)
  int g_seg_cols;                  // short-reduction kernel: G's columns in segments g_seg_stride elements apart
  long g_seg_stride;               //   (P same-shaped gradient tensors side by side); 0 = plain [M, N1]
  int Hs, Ws, Cs, Hd, Wd, kh, kw, stride, pad;
  float* ws;                       // gemm_tn_big.hip: per-(split, tile) partial tiles, summed by a second launch; or NULL
  float* ws_caller;                // the caller's workspace (fod_gemm_tn_acc / fod_conv2d_wgrad_acc `ws`), ws_caller_bytes long
  size_t ws_caller_bytes;
  // Deterministic forms (`_det` entry points) only; zero otherwise.  det = 1: nothing is added with atomics -- a launch
  // that cannot place its partial results in the caller's workspace fails instead.
  int det;
  float* part;                     // gemm_tn.hip: partial s = part + s * part_stride: [N1 * K2] tile sums, then [N1] column sums
  long part_stride;
  float* part_cs;                  // gemm_tn_big.hip: partial column sums [nsplit * waves along j][N1]
};

constexpr int MSTEP = 32;   // gemm_tn.hip: reduction rows per step of the 128 x 128 kernel
constexpr int MS = 64;      // gemm_tn_big.hip: reduction rows per stage

// Operand extents in bytes, which the host checks against 4 GiB before they go into the buffer descriptors.  G: [M, N1], or
// its N1 columns in segments of g_seg_cols that lie g_seg_stride elements apart (0 = plain); X: [M, K2].  (The job kernels
// form the same extents from their table entries in place: profiles/tn_shared_pieces_isa.txt.)
inline long g_extent(int M, long ldg, int N1, int g_seg_cols, long g_seg_stride, long esz) {
  const long nseg = g_seg_cols > 0 ? (N1 + g_seg_cols - 1) / g_seg_cols : 1;
  const long seg_c = g_seg_cols > 0 ? g_seg_cols : N1;
  return ((nseg - 1) * g_seg_stride + (long)(M - 1) * ldg + seg_c) * esz;
}
inline long x_extent(int M, long ldx, int K2, long esz) { return ((long)(M - 1) * ldx + K2) * esz; }

// Which kernel takes a weight gradient and how (tile, M-splits, block order, where the partial results go): decided by
// route() (gemm_tn.hip) from the checked parameters -- p.det and the caller's workspace among them -- and a snapshot of
// the knobs, and by nothing else; the launchers only launch what it says.
typedef fod_tn_route TnRoute;
TnRoute route(int mode, int dtype, const TnParams& p, const Knobs& kn);
// gemm_tn_big.hip: r.kernel == FOD_ROUTE_TN_BIG, the 8-wave LDS-DMA kernel for long bf16 reductions (conv weight
// gradients, the encoder's Linear weight gradients)
int launch_big(int mode, const TnParams& p, const TnRoute& r, hipStream_t stream);
// the FOD_CONV_WGRAD half of fod_conv2d_route
int conv_wgrad_route(int dtype, const fod_conv_geom* g, int det, size_t ws_bytes, fod_tn_route* out);

}  // namespace fodtn
