"""Every torch.autograd.Function of future_od/native/functional.py and future_od/native/backbone.py and the float64 cases
that check its gradients: ONE table, read by tests/test_autograd_census_cpu.py (the classes found in the two source files
must be exactly the keys of NODES, every case named here must exist, every test cited must exist -- no GPU needed) and by
tests/test_autograd_nodes_gpu.py (which runs every case of CASES against float64 torch autograd on the CPU).

The rule: a new autograd node gets an entry in NODES -- the names of its cases in tests/test_autograd_nodes_gpu.py, or, if a
test already compares its gradients with torch / float64 (not with another path of this project), that test.

Data only: no torch, nothing is computed here."""
from collections import namedtuple

BOTH = ("f32", "bf16")
BF16 = ("bf16",)

# limits on ||got - ref||_2 / ||ref||_2 per compared slice: f32 -- the per-kernel bound is 2e-5 (tol() of
# tests/test_kernels_gpu.py) and no node chains more than five kernels; bf16 -- one rounding has a relative RMS of about
# 2e-3 and a single node stores at most three rounded tensors between an input and a gradient
LIMIT = {"f32": 1e-4, "bf16": 1e-2}
MEASURED_FACTOR = 3.0       # kernel summation order and f32 atomics come on top of the roundings that can be modelled

# name:     the case (a class of that name in tests/test_autograd_nodes_gpu.py); the inputs are seeded from it
# dtypes:   the compute dtypes it runs in ("bf16" alone: the node, or the branch, exists only there)
# measured: None -- a single node, LIMIT applies.  A number -- a CHAIN of nodes that stores more than three bf16 tensors
#           between an input and a gradient: the largest error, over the compared slices, of the case's float64 reference
#           with a bf16 rounding at every tensor the nodes store (activations and gradients) against the same reference
#           without; measured on the CPU by `python tests/test_autograd_nodes_gpu.py` (no GPU is needed for it), and the
#           bf16 limit of the case is MEASURED_FACTOR times it.  In f32 a chain keeps LIMIT["f32"].  A dict -- the same
#           per slice, where one figure for the whole case would be far too wide for most of its slices (imu_mlp).
#           tests/test_autograd_limits_cpu.py measures again and fails when the table no longer says what it gets.
Case = namedtuple("Case", "name dtypes measured")
CASES = {}


def _case(name, dtypes=BOTH, measured=None):
    assert name not in CASES, name
    CASES[name] = Case(name, tuple(dtypes), measured)
    return name


def limit(name, dtype, what=""):
    """The limit of slice `what` ("out y", "d w[q]", ...) of a case."""
    c = CASES[name]
    if dtype == "bf16" and c.measured is not None:
        m = c.measured
        return MEASURED_FACTOR * (m.get(what, m[""]) if isinstance(m, dict) else m)
    return LIMIT[dtype]


CoveredElsewhere = namedtuple("CoveredElsewhere", "target")       # target: "<test file>::<test function>"


def COVERED_ELSEWHERE(target):
    return CoveredElsewhere(target)


# ------------------------------------------------------------------------------------------------ single nodes
_case("linear_plain")
_case("linear_relu")
_case("linear_out_f32")
_case("linear_n2")                       # N = 2 (ref_point_head's output): the padded gradient, dw[:N] / db[:N]
_case("linear_shared_twice")             # one layer on two inputs: the second use joins the first's job (WGRADS.chain)
_case("keep_plain")                      # the returned x is consumed too: dkeep rides in the input-gradient GEMM
_case("keep_relu")
_case("keep_fallback_n2")                # N % vec != 0: two consumers, no LinearKeepFn
_case("add_same")
_case("add_row_mod")
_case("add_row_div")
_case("mul_same")
_case("mul_row_mod")
_case("expand_rows3")
_case("cast_pad")                        # f32 -> compute dtype, pad_cols > cols
_case("cast_noop")
_case("ln_plain")
_case("ln_res_same")
_case("ln_res_div")                      # residual [F, D] over N tokens each: the plain colsum_acc path
_case("ln_stacked")                      # the decoder's shared output norm over all levels at once
_case("lan_then_pre1", BF16)             # LinearAddNormFn(then=...), FOD_FUSED_LINEAR_PRE=1: the second result is differentiable
_case("lan_then_pre0", BF16)             # ... =0: a constant that LinearKeepFn(precomputed=...) adopts
_case("attn_two_part_cross")             # S != T, q2 / k2: no slot layout
_case("group_unused_output")             # P = 3, the second output unused: separate gradients (one of zeros), _gather_segments
_case("wide_p4")
_case("wide_p4_table")                   # the input has no gradient (the positional table)
_case("mlp2_shared3", BF16)              # three calls, one TableGradAcc, the first hands the total on
_case("mlp2_single", BF16)
_case("imu_plain", BF16)                 # ImuBranchFn, use_mlp = False, no queue
_case("zero_grad_anchor")
_case("refpoint_both")                   # RefPointSineFn.apply: ref and sine both consumed
_case("refpoint_ref_only")               # only ref consumed: the dsine-is-None zeros
_case("refpoint_sine_only")              # only sine consumed: dref is None
_case("box_finish_shared_points")        # BoxFinishFn.apply: t [Lv, B * M, 4], row r uses ref[r % M]
_case("refpoint_into_boxes")             # ref of the first node into the second: dref comes back as dref_extra


# ------------------------------------------------------------------------------------------------ chains of nodes
# (measured: see Case; the figures are printed by `python tests/test_autograd_nodes_gpu.py`)
_case("ffn_masked_tail", measured=2.72e-03)            # LinearKeepFn(grad_masked) -> LinearAddNormFn(a_relu)
_case("in_proj_attn", measured=4.11e-03)               # InProjFn -> AttentionFn: q | k column siblings
_case("in_proj_self_table", measured=6.47e-03)         # InProjSelfFn, pos a [N, D] table, src also feeds a residual
_case("in_proj_self_tensor", measured=6.31e-03)        # ... pos [F, N, D]
_case("in_proj_self_no_input_grad", measured=6.43e-03)
_case("in_proj_cross", measured=4.15e-03)              # three inputs, the key input without gradient
_case("group_attn_self", measured=3.73e-03)            # GroupLinearFn -> AttentionFn: dq | dk | dv as buf[0..2] (_as_segments)
_case("group_res_rows_bm", measured=2.47e-03)          # tables from an earlier group_linear, rows = B * M
_case("group_res_rows_m", measured=2.05e-03)           # ... rows = M
# ImuBranchFn, use_mlp: value -> out_proj -> norm1 -> MLP -> norm2.  Measured PER SLICE: the bf16 rounding of norm1's output
# flips a few ReLU units of the MLP (5 rows x 512 units; each flip moves a gradient by that unit's whole term), which
# dominates every gradient upstream of the ReLU in blocks 1 and 2 and none of the others ("": every slice not listed)
_case("imu_mlp", BF16, measured={
    "": 6.90e-03, "d ego": 3.37e-02,
    "d wv1": 3.00e-02, "d bv1": 2.50e-02, "d wo1": 2.93e-02, "d bo1": 2.66e-02, "d g11": 2.88e-02, "d e11": 2.63e-02,
    "d w01": 4.88e-02, "d b01": 4.58e-02,
    "d wv2": 4.57e-02, "d bv2": 4.22e-02, "d wo2": 4.53e-02, "d bo2": 4.49e-02, "d g12": 4.88e-02, "d e12": 4.40e-02,
    "d w02": 6.74e-02, "d b02": 6.74e-02})
_case("imu_queue_norms", BF16, measured=3.26e-03)      # ImuBranchFn + three LayerNormFn(res_queue=...) on its results
# the memory side of the decoder: wide_linear per image and of the positional table, MemorySide, L x K hoisted
# cross-attention calls.  n42: fod_attn_bwd writes the slots; n272 (bf16): the _DkvQueue.  shared: ks_all [N, L*K*D];
# per_batch: [B, N, L*K*D] (the positional encoding with its temporal term)
_case("memory_n42_shared", measured=3.74e-03)
_case("memory_n42_per_batch", measured=3.52e-03)
_case("memory_n272_shared", BF16, measured=3.85e-03)
_case("memory_n272_per_batch", BF16, measured=3.63e-03)


# ------------------------------------------------------------------------------------------------ the nodes
_K = "tests/test_kernels_gpu.py::"
_H = "tests/test_heads_gpu.py::"
_MEMORY = ["memory_n42_shared", "memory_n42_per_batch", "memory_n272_shared", "memory_n272_per_batch"]
NODES = {
    "LinearFn": ["linear_plain", "linear_relu", "linear_out_f32", "linear_n2", "linear_shared_twice", "keep_fallback_n2"],
    "LinearKeepFn": ["keep_plain", "keep_relu", "ffn_masked_tail", "lan_then_pre0"],
    "AddFn": ["add_same", "add_row_mod", "add_row_div"],
    "MulFn": ["mul_same", "mul_row_mod"],
    "Mlp2MulFn": ["mlp2_shared3", "mlp2_single"],
    "ExpandRowsFn": ["expand_rows3"],
    "LayerNormFn": ["ln_plain", "ln_res_same", "ln_res_div", "ln_stacked", "imu_queue_norms"],
    # without `then`: the float64 half of the test named first; here a_relu and the two then forms
    "LinearAddNormFn": ["ffn_masked_tail", "lan_then_pre1", "lan_then_pre0"],
    "ConvFn": COVERED_ELSEWHERE(_K + "test_same_padded_dilated_conv_with_gradients"),
    # the same test: dilations 2, 4 and 8 against F.conv2d(dilation=d), one image with H = 7 < d = 8
    "_ScatterGridFn": COVERED_ELSEWHERE(_K + "test_same_padded_dilated_conv_with_gradients"),
    "DropoutFn": COVERED_ELSEWHERE(_H + "test_dropout_is_stateless_and_self_consistent"),
    "AttentionFn": ["in_proj_attn", "group_attn_self", "attn_two_part_cross", "in_proj_cross"],
    "InProjFn": ["in_proj_attn"],
    "InProjSelfFn": ["in_proj_self_table", "in_proj_self_tensor", "in_proj_self_no_input_grad"],
    "InProjCrossFn": ["in_proj_cross"],
    # (tests/test_heads_gpu.py::test_refpoint_sine_and_box_finish and its layout variant hold the KERNELS of these two
    # against torch through ops.*; they never apply the Functions, so the nodes have cases of their own)
    "RefPointSineFn": ["refpoint_both", "refpoint_ref_only", "refpoint_sine_only", "refpoint_into_boxes"],
    "BoxFinishFn": ["box_finish_shared_points", "refpoint_into_boxes"],
    "ZeroGradAnchor": ["zero_grad_anchor"],
    "CastFn": ["cast_pad", "cast_noop"],
    "WideLinearFn": ["wide_p4", "wide_p4_table"] + _MEMORY,
    "GroupLinearFn": ["group_attn_self", "group_res_rows_bm", "group_res_rows_m", "group_unused_output"],
    "ImuBranchFn": ["imu_plain", "imu_mlp", "imu_queue_norms"],
    "HoistedCrossAttnFn": _MEMORY,
    "BackboneFn": COVERED_ELSEWHERE("tests/test_model_gpu.py::test_fp32_parity_with_oracle_and_golden"),
}
# LinearAddNormFn without `then` and without a_relu is not a case here: the second half of
# tests/test_kernels_gpu.py::test_fused_linear_add_norm_backward holds the node against float64 torch autograd
ALSO_COVERED = [_K + "test_fused_linear_add_norm_backward"]
