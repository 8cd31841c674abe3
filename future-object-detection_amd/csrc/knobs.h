// The kernel-selection knobs of libfod_hip.so: ONE table, read from the environment once.
//
// Every FOD_* variable the library itself looks at has a field here, with its default.  The table is filled at its first
// use in the process (values are parsed and copied; nothing points into the environment afterwards) and changed only by
// fod_knob_set (include/fod.h), so a variable exported after the first launch is not seen.  It is process-wide HOST
// state behind a mutex: launchers take a snapshot (fod_knobs()) and hand it to the pure route functions of gemm_nt.h /
// gemm_tn.h.  No device state is involved, and a captured graph has the routes of its capture baked in -- changing a
// knob does not change what a replay runs.
//
// What the values were measured to do is written where they are used (the route functions and the launchers).
#pragma once

struct Knobs {
  static constexpr int AUTO = -1;   // "not set": the rule in the comment decides
  // ---- NT contractions (gemm_nt.hip, gemm_nt_big.hip)
  int nt_small = 1;            // FOD_NT_SMALL        0: never the short-launch 64 x 64 kernel
  int nt_narrow = AUTO;        // FOD_NT_NARROW       n: 64-wide tiles below n 128-wide ones, fill rule off; auto: 320 + fill rule
  int nt_splitk = AUTO;        // FOD_NT_SPLITK       0: never split K; n > 1: at most n (<= 8) splits; auto: at most 4
  int nt_big = 1;              // FOD_NT_BIG          0: never the 256-row LDS-DMA kernel, 2: whenever legal (tests), 1: large problems
  int nt_big256 = 1;           // FOD_NT_BIG256       0: never its 256 x 256 tile, 2: whenever N >= 256 (tests), 1: where it fills the chip
  int nt_big_ilv = AUTO;       // FOD_NT_BIG_ILV      0 / 1: interleaved DMA requests off / on; auto: on with the three-stage ring only
  int nt_big256_mink = 128;    // FOD_NT_BIG256_MINK  contraction depth from which convolutions take the 256 x 256 tile
  int nt_big_mink = 1536;      // FOD_NT_BIG_MINK     contraction depth from which the 256 x 128 tile is taken
  int nt_big_minn = 256;       // FOD_NT_BIG_MINN     ... and output width
  // ---- TN contractions: weight gradients (gemm_tn.hip, gemm_tn_big.hip)
  int tn_small = 1;            // FOD_TN_SMALL        0: never the short-reduction 64 x 64 kernel
  int tn_big = 1;              // FOD_TN_BIG          0: never the 8-wave LDS-DMA kernel, 2: whenever legal (tests; Linear layers too), 1: long reductions
  int tn_big_dense = 0;        // FOD_TN_BIG_DENSE    1: Linear weight gradients may take it too
  int tn_big256 = 0;           // FOD_TN_BIG256       1: its 256 x 256 tile on multiples of 256 with M >= 16384, 2: whenever N1, K2 >= 256 (tests)
  double tn_big_min = 2.0e9;   // FOD_TN_BIG_MIN      M * N1 * K2 from which it is taken
  int tn_big_splits = 0;       // FOD_TN_BIG_SPLITS   n > 0: its number of M-splits; 0: planned
  int tn_ws = 1;               // FOD_TN_WS           0: f32 atomics straight into dW although a workspace was handed over
  int tn_xcd = 1;              // FOD_TN_XCD          0: plain block order instead of one XCD per M-split
  int tn_rows = 0;             // FOD_TN_ROWS         n > 0: rows per M-split of the 128 x 128 kernel; 0: planned
  // ---- the others only keep their switch here
  int attn_lds = 8;            // FOD_ATTN_LDS        0: no LDS-staged attention kernels, 4: four-wave forward, 8: eight-wave forward
  int attn_pf = 1;             // FOD_ATTN_PF         0: no prefetching dK/dV kernel
  int fp8_stage = 1;           // FOD_FP8_STAGE       2: two 64-key tiles per barrier in the fp8 attention forward
  int ln_bwd_groups = 4;       // FOD_LN_BWD_GROUPS   row groups (1..16) a wave of the many-row layer-norm backward walks
  int bnk_version = 4;         // FOD_BNK_VERSION     2: one tile per workgroup in the fused bottleneck; 4: persistent workgroups
};

// A snapshot of the table (api.cpp).
Knobs fod_knobs();
