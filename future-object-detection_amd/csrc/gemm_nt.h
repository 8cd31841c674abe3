// Shared between gemm_nt.hip (128-row tiles, register-staged ring) and gemm_nt_big.hip (256-row tiles, LDS-DMA ring).
#pragma once
#include "common.h"
#include "knobs.h"

namespace fodnt {

enum { MODE_DENSE = 0, MODE_CONV = 1, MODE_DGRAD = 2, MODE_DGRAD_S2 = 3, MODE_STEM = 4 };

struct NtParams {
  const void* A;
  const void* B;
  void* C;
  long lda, ldb, ldc;
  int M, N, K;
  int a_row_mod;
  const float* scale;
  const float* shift;
  const void* res;
  long ldr;
  int res_row_mod;
  const void* mask;
  long ldmask;
  int relu;
  int c_is_f32;
  int vec_epi;   // host-checked: N, ldc, ldr, ldmask multiples of 4 and 16-byte aligned bases
  unsigned a_bytes, b_bytes;   // extents of A and B for the buffer descriptors (< 4 GiB, host-checked)
  int gx, gy;                  // tile grid (n-tiles, m-tiles); launched as a 1-D grid of gx * roundup(gy, 8)
  // grouped form (short-launch kernel only): A's k range and C's columns are cut into segments that live
  // a_seg_stride / c_seg_stride elements apart -- P same-shaped tensors side by side without a concatenation
  int a_seg_len, c_seg_cols;   // elements per segment; 0 = not segmented
  long a_seg_stride, c_seg_stride;
  // MODE_DGRAD_S2: class geometry.  m indexes (img, hi', wi') of the class grid Hd x Wd; hi = 2*hi' + par_h
  int par_h, par_w, out_H, out_W;   // parity of the class, full input dims (rows of C / residual / mask)
  int r_first, s_first, n_s;        // first valid tap per axis, taps per row of the compact list
  int off_h, off_w;                 // source row = hi' + off_h - ri
  // short-launch kernel: K split ACROSS blocks (gridDim.z = ksplit); partial 64 x 64 f32 tiles meet in split_ws, the
  // block that draws the last ticket sums them in index order and runs the epilogue
  int ksplit;
  float* split_ws;
  unsigned* split_tickets;
  // short-launch kernel, batched form (fod_gemm_nt_batched): `batches` independent problems of one shape in one launch;
  // blockIdx.y = batch * m-tiles + m-tile; operand b of batch z starts *_batch elements after that of batch z - 1
  int batches;
  long a_batch, b_batch, c_batch, shift_batch, res_batch, mask_batch;
  // grouped form: the residual of C's column segment s < res_nseg is block s of a [res_nseg][*, c_seg_cols] operand whose
  // blocks lie res_seg_stride elements apart (row(m) as usual); segments >= res_nseg get none.  res_nseg = 0: one
  // [*, N] residual for all columns
  int res_nseg;
  long res_seg_stride;
  // gather geometry
  int Hs, Ws, Cs;   // source image dims / channels
  int Hd, Wd;       // m-domain dims
  int kh, kw, stride, pad;
};

constexpr int BM = 128;
constexpr int ROW_BYTES = 128;   // bytes of k per tile row

FOD_DEVINL int lds_off(int row, int chunk) { return row * ROW_BYTES + ((chunk ^ ((row >> 1) & 7)) << 4); }

constexpr int BMB = 256, BKB_EL = 64;   // gemm_nt_big.hip: rows and k elements of its tiles

// Operands are read with raw buffer loads: an out-of-range chunk (row tail, k tail, conv padding) gets the
// byte offset OOB, which the hardware range check turns into zeros -- no branch and no select around
// the load, so hipcc keeps counted vmcnt waits and the staged tile stays in flight during the MFMAs.
constexpr unsigned OOB = 0xFFFFFFF0u;

// XCD-aware tile order.  Workgroups are dealt round-robin over the 8 XCDs (private L2 each), so block
// ids congruent mod 8 share an L2: give each XCD whole m-tiles (all of an m-tile's n-tiles re-read the
// same gathered A rows; neighbouring m-tiles share 3x3 halo rows) instead of striping n-tiles over XCDs.
struct TileOrigin {
  int m0, n0;
  bool ok;   // false: this block is padding of the grid (gy rounded up to 8) and has no tile
};
template <int TILE_M, int TILE_N>
FOD_DEVINL TileOrigin tile_origin(const NtParams& p) {
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int nt_i = slot % p.gx;
  const int mt_i = (slot / p.gx) * 8 + xcd;
  return TileOrigin{mt_i * TILE_M, nt_i * TILE_N, mt_i < p.gy};
}

// Pixel (img, h, w) of the m-domain Hd x Wd: a thread's (lane's) first row by division, its later rows (+STEP tile
// rows each) by stepping: eight 32-bit divisions per thread were ~0.5 us of every block's prologue
struct PixelWalk {
  int img, h, w;
  FOD_DEVINL PixelWalk(const NtParams& p, int mfirst) {
    const int hw = p.Hd * p.Wd;
    img = mfirst / hw;
    const int rem = mfirst - img * hw;
    h = rem / p.Wd;
    w = rem - h * p.Wd;
  }
  // this row's pixel; the walk moves on to the thread's next row
  template <int STEP>
  FOD_DEVINL PixelWalk next(const NtParams& p) {
    const PixelWalk here = *this;
    w += STEP;
    while (w >= p.Wd) {
      w -= p.Wd;
      if (++h == p.Hd) {
        h = 0;
        ++img;
      }
    }
    return here;
  }
};

// Gather origin (a_h, a_w) of the row at pixel px in the three conv modes (tap_source below adds or subtracts the tap);
// a row past M gets an a_h that fails every bounds test.  Returns the byte offset of the row's image.
template <int MODE, unsigned ESZ>
FOD_DEVINL unsigned row_origin(const NtParams& p, const PixelWalk& px, bool valid, int& a_h, int& a_w) {
  const unsigned img_base = (unsigned)((long)px.img * p.Hs * p.Ws * p.Cs * (long)ESZ);
  if (MODE == MODE_CONV) {
    a_h = valid ? px.h * p.stride - p.pad : -(1 << 28);
    a_w = px.w * p.stride - p.pad;
  } else if (MODE == MODE_DGRAD_S2) {
    a_h = valid ? px.h + p.off_h : -(1 << 28);
    a_w = px.w + p.off_w;
  } else {
    a_h = valid ? px.h + p.pad : -(1 << 28);
    a_w = px.w + p.pad;
  }
  return img_base;
}
// Byte offset of source pixel (a_h, a_w) inside its image (modulo 2^32 for negative coordinates: only used after the
// bounds check).  Added to the image offset, and to the byte offset of the caller's 16-byte chunk, it gives a row base
// to which a tap adds (forward) or subtracts (dgrad modes) one block-uniform delta, UniformTapWalk::off
template <unsigned ESZ>
FOD_DEVINL unsigned origin_offset(const NtParams& p, int a_h, int a_w) {
  return ((unsigned)a_h * (unsigned)p.Ws + (unsigned)a_w) * (unsigned)p.Cs * ESZ;
}

// Block-uniform tap walk (r, s, c) of the tile being requested (tiles come in increasing order), for channel counts
// that are a multiple of the tile's k elements: a k-tile lies inside ONE tap, c = the tile's first channel, the state
// lives in SGPRs and costs scalar instructions.
//   off = ((r * Ws + s) * Cs +- c) * ESZ is the source-side byte delta of (tap (r, s), channel c): added to the
//         row's base in the forward conv, subtracted (taps walk backwards, the channel still counts up) in both
//         dgrad modes.
//   kb  (MODE_DGRAD_S2) = byte offset of (full-kernel tap, c) in a weight row: the class contracts over a compact
//         tap list of n_s taps per row that starts at (r_first, s_first) and takes every second tap.
// Everything advances by adds.
template <int MODE, unsigned ESZ>
struct UniformTapWalk {
  int tap_w;                            // taps per row of the list that is walked
  unsigned row_skip, kb_row_skip, cs_b;
  int r = 0, s = 0, c = 0;
  unsigned off = 0, kb = 0;
  FOD_DEVINL explicit UniformTapWalk(const NtParams& p) {
    tap_w = MODE == MODE_DGRAD_S2 ? p.n_s : p.kw;
    row_skip = (unsigned)((p.Ws - tap_w) * p.Cs) * ESZ;
    kb_row_skip = (unsigned)((2 * p.kw - 2 * tap_w) * p.Cs) * ESZ;
    cs_b = (unsigned)p.Cs * ESZ;
    if (MODE == MODE_DGRAD_S2) kb = (unsigned)((p.r_first * p.kw + p.s_first) * p.Cs) * ESZ;
  }
  template <int BK_EL>   // k elements per tile
  FOD_DEVINL void advance(const NtParams& p) {
    constexpr unsigned BKB = BK_EL * ESZ;
    c += BK_EL;
    off = MODE == MODE_CONV ? off + BKB : off - BKB;
    kb += BKB;
    if (c >= p.Cs) {                              // at most once: Cs % BK_EL == 0
      c -= p.Cs;
      if (MODE != MODE_CONV) off += 2 * cs_b;     // (s+1)*Cs - (c-Cs) vs s*Cs - c; forward: the sum is unchanged
      kb += cs_b;                                 // the full kernel advances by two taps
      if (++s == tap_w) {
        s = 0;
        ++r;
        off += row_skip;
        kb += kb_row_skip;
      }
    }
  }
};

// Source pixel (hs, ws) of tap (r, s) for a row with origin (a_h, a_w) -- forward: origin + tap; both dgrad modes walk
// the taps backwards -- and whether the chunk is read: k inside K (k_in), pixel inside the image (no padding, row < M)
template <int MODE>
FOD_DEVINL bool tap_source(const NtParams& p, bool k_in, int a_h, int a_w, int r, int s, int& hs, int& ws) {
  hs = MODE == MODE_CONV ? a_h + r : a_h - r;
  ws = MODE == MODE_CONV ? a_w + s : a_w - s;
  return k_in && (unsigned)hs < (unsigned)p.Hs && (unsigned)ws < (unsigned)p.Ws;
}
// row of C / residual / mask for tile row m (identity except for the parity-class launches)
template <int MODE>
FOD_DEVINL long out_row(const NtParams& p, int m) {
  if (MODE != MODE_DGRAD_S2) return m;
  const int hw = p.Hd * p.Wd;
  const int img = m / hw;
  const int rem = m - img * hw;
  const int hq = rem / p.Wd;
  const int wq = rem - hq * p.Wd;
  return ((long)img * p.out_H + 2 * hq + p.par_h) * p.out_W + 2 * wq + p.par_w;
}

// ---- row epilogue (vec_epi): a lane owns columns n .. n + 3 of a row; nc = min(n, N - 4) clamps what is only read.
// residual / mask segments of tile row mt, clamped to the last row: no branch around the loads, so a batch of rows can
// be requested up front
template <int MODE, typename T, typename VT>
FOD_DEVINL void fetch_res_mask(const NtParams& p, const T* Rp, const T* Mp, bool has_res, bool has_mask, int mt, int nc,
                               VT& rres, VT& rmsk) {
  const long m = out_row<MODE>(p, min(mt, p.M - 1));
  if (has_res) {
    const long rm = p.res_row_mod > 0 ? (m % p.res_row_mod) : m;
    rres = *reinterpret_cast<const VT*>(Rp + rm * p.ldr + nc);
  }
  if (has_mask) rmsk = *reinterpret_cast<const VT*>(Mp + m * p.ldmask + nc);
}
// scale/shift, residual, relu, relu-mask in this order, the options chosen at compile time: straight-line code, no
// option costs instructions when it is off
template <bool HAS_RES, bool DO_RELU, bool HAS_MASK, typename VT>
FOD_DEVINL f32x4 epilogue4(const f32x4& v, const f32x4& sc, const f32x4& sh, const VT& rres, const VT& rmsk) {
  f32x4 w = v * sc + sh;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (HAS_RES) w[e] += (float)rres[e];
    if (DO_RELU) w[e] = fmaxf(w[e], 0.f);
    if (HAS_MASK) w[e] = ((float)rmsk[e] > 0.f) ? w[e] : 0.f;
  }
  return w;
}
FOD_DEVINL void store4(const NtParams& p, bool as_f32, long mo, int n, const f32x4& w) {
  if (as_f32) {
    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + mo * p.ldc + n) = w;
  } else {
    *reinterpret_cast<bf16x4_t*>(reinterpret_cast<__bf16*>(p.C) + mo * p.ldc + n) =
        bf16x4_t{(__bf16)w[0], (__bf16)w[1], (__bf16)w[2], (__bf16)w[3]};
  }
}

// Which kernel takes a problem and how: decided by route() (gemm_nt.hip) from the checked parameters and a snapshot of
// the knobs, and by nothing else -- the launchers below only launch what it says.
typedef fod_nt_route NtRoute;
NtRoute route(int mode, int dtype, const NtParams& p, const Knobs& kn);
// gemm_nt_big.hip: r.kernel == FOD_ROUTE_NT_BIG
int launch_big(int mode, const NtParams& p, const NtRoute& r, hipStream_t stream);

}  // namespace fodnt
