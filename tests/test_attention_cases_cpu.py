"""tests/attention_cases.py without a GPU: the conditions its problems are built to meet, the error budgets under a torch
emulation of the kernels' roundings, mutants that the budgets reject -- and the same mutants accepted by the bound the
Gaussian-input tests use, at the long key sequences the model runs.

The conditions are properties of the operands, not measurements:
  * every operand, and bf16(0.125 q), is held exactly (for the shapes that also run on the fp8 forward: by MX e4m3 too);
  * every key is detectable pass by pass: left out of the forward's softmax it moves some element of o by 8 tolerances
    (analytically: delta o_i = p_ij / (1 - p_ij) (o_i - v_j)); left out of the dq pass, which takes lse2 and delta from
    the forward, its term moves some element of dq1 (dq2) by 8 tolerances; left out of the dk / dv pass its own rows of
    dk1 (dk2) and dv, which vanish, stand 8 tolerances above zero -- for some call of the case;
  * every query row left out of the dk / dv sums moves some element of dv by 8 tolerances, for some call of the case;
  * the flat profile's unit is an aligned run of 32 keys; the fp8 forward's factor is 2 (P in e4m3 costs 2^-4).
Under dropout a dropped probability carries nothing: a key is asked of o / dq where a query that targets it keeps it."""
import math

import pytest
import torch

import attention_cases as AC
import variant_cases as V
from test_kernels_gpu import _mx_e4m3, rnd

SHAPES = AC.shapes()
DEMO = [(2, 8, 128, 1450, 2), (1, 1, 33, 2000, 2)]


def _sid(sp):
    return "x".join(map(str, sp[0])) + "-" + sp[1]


def test_the_scale_makes_the_score_factor_a_power_of_two():
    assert AC.exact_scale_products() == [0.25, 0.125, 0.0625]
    assert float(torch.tensor(AC.SCALE, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)) == 0.125


def test_the_case_list_covers_what_it_promises():
    runs = AC.runs()
    assert len({AC.run_id(c, prof) for c, prof in runs}) == len(runs)
    table = {c.shape for c, _ in runs}
    for fam in ("attn_family", "attn_ksplit", "attn_strided"):
        assert all(c.shape in table for c in V.cases(fam))
    for shape in V.ATTN_FWD_BWD_SHAPES:
        for dt in V.BOTH:
            assert any(c.shape == shape and c.dtype == dt and not c.knobs for c, _ in runs), (shape, dt)
    assert {c.shape[2] for c, _ in runs} >= set(V.ATTN_EDGE_TQ) and {c.shape[3] for c, _ in runs} >= set(V.ATTN_EDGE_S)
    assert any(c.shape[3] % 128 == 1 and c.shape[3] > 128 for c, _ in runs)
    drops = [c for c, prof in runs if prof == "dropout"]
    for dt in V.BOTH:
        assert {bool(c.knobs) for c in drops if c.dtype == dt} == {False, True}
    assert max(c.shape[2] for c, _ in runs) <= 700 and max(c.shape[3] for c, _ in runs) <= 2000      # nothing larger than before
    # every route the library can report for bf16 and f32 is some case's (fwd / dq / dkv family, key split, dropout)
    names = {AC.route_name(c).split("-ks")[0] for c, _ in runs}
    assert {"bf16:lds8/lds/lds", "bf16:lds4/lds/lds", "bf16:plain/plain/prefetch", "bf16:plain/plain/plain",
            "bf16:split/split/prefetch", "bf16:split/split/plain", "f32:plain/plain/plain", "f32:split/split/plain",
            "bf16:plain/plain/prefetch-drop", "bf16:plain/plain/plain-drop", "bf16:split/split/prefetch-drop",
            "bf16:split/split/plain-drop", "f32:plain/plain/plain-drop", "f32:split/split/plain-drop"} <= names, sorted(names)
    assert any("-ks" in AC.route_name(c) and c.extra.get("drop") for c, _ in runs)
    assert any("-ks" in AC.route_name(c) and c.dtype == "f32" for c, _ in runs)


@pytest.mark.parametrize("sp", SHAPES, ids=_sid)
def test_conditions_and_budgets(sp):
    shape, profile = sp
    B, H, Tq, S, parts = shape
    fp8 = profile != "dropout" and shape in AC.fp8_shapes()
    for call in range(AC.n_calls(shape, profile)):
        p = AC.problem(shape, profile, call)
        assert AC.round_trips(p)
        if fp8:
            _survives_mx_e4m3(p)
        # the emulated roundings stay inside the budgets (both ways of summing the normaliser); A = 0 forces 0
        for lds in (False, True):
            worst = AC.assert_within(p, AC.emulate_bf16(p, lds), "bf16", f"emulation, lds={lds}, {shape}")
            assert max(worst.values()) <= 1.0
    if profile == "flat":
        assert float(AC.problem(shape, "flat").ref["dk1"].abs().max()) == 0.0
        assert float((AC.problem(shape, "flat").ref["lse2"] - math.log2(S)).abs().max()) <= 1e-12
        for seen in [AC.flat_detection(shape)] + ([AC.flat_detection(shape, o_factor=AC.FP8_FACTOR["o"], detect=2.0)] if fp8 else []):
            for name, hit in seen.items():
                assert bool(hit.all()), (shape, name, hit.tolist())
    elif S >= 2:
        for kw in [{}] + ([dict(o_factor=AC.FP8_FACTOR["o"], detect=2.0)] if fp8 else []):
            seen, rows, need, need_rows = AC.pointer_detection(shape, profile, **kw)
            for name in seen:
                assert bool((seen[name] | ~need[name]).all()), (shape, profile, name, int((need[name] & ~seen[name]).sum()))
                if profile == "pointer":
                    assert bool(need[name].all()), (shape, name)                    # every key is some query's target
                else:       # keep = 1/2 per probability, two calls or more: 3/4 of the keys and of the rows are expected
                    assert float(need[name].float().mean()) >= 0.5
            assert bool((rows | ~need_rows).all()), (shape, profile, int((need_rows & ~rows).sum()))
            assert bool(need_rows.all()) if profile == "pointer" else float(need_rows.float().mean()) >= 0.7


def _survives_mx_e4m3(p):
    H = p.shape[1]
    hd = lambda t: AC.heads(t.float(), H)
    for name, t, dim in (("q1", p.q1 * 0.125, -1), ("k1", p.k1, -1), ("v", p.v, -2), ("q2", None if p.q2 is None else p.q2 * 0.125, -1),
                         ("k2", p.k2, -1)):
        if t is not None:
            assert float(t.abs().max()) <= 24 and torch.equal(_mx_e4m3(hd(t), dim), hd(t).contiguous()), (p.shape, p.profile, p.call, name)


@pytest.mark.parametrize("shape", AC.fp8_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_fp8_shapes_survive_the_quantiser(shape):
    """(Shapes of the fp8 runs that are not in the table of cases: their operands round-trip, their keys are detectable.)"""
    for profile in ("pointer", "flat"):
        for call in range(2 if profile == "pointer" else 1):
            p = AC.problem(shape, profile, call)
            assert AC.round_trips(p)
            _survives_mx_e4m3(p)
    if shape[3] >= 2:
        seen, _, need, _ = AC.pointer_detection(shape, "pointer", o_factor=AC.FP8_FACTOR["o"], detect=2.0)
        assert bool((seen["o"] | ~need["o"]).all()) and bool(need["o"].all())
        assert all(bool(hit.all()) for hit in AC.flat_detection(shape, o_factor=AC.FP8_FACTOR["o"], detect=2.0).values())


# ------------------------------------------------------------------------------------------------ mutants
def _mutants(shape, active_row):
    """{name: (w, rw)}: key weights [1,1,1,S] and query-row weights [1,1,Tq,1] of the mutated attention."""
    B, H, Tq, S, parts = shape
    ones = lambda: torch.ones(1, 1, 1, S, dtype=torch.float64)
    out = {}
    w = ones(); w[..., S - 1] = 0.0
    out["last key removed"] = (w, None)
    if S > 32:
        w = ones(); w[..., S - 32 - S % 32:S - S % 32] = 0.0
        out["an aligned run of 32 keys removed"] = (w, None)
    if S > 128:
        w = ones(); w[..., 64:128] = 0.0
        out["keys 64..127 removed"] = (w, None)
    w = ones(); w[..., S // 2] = 2.0
    out["one key counted twice"] = (w, None)
    rw = torch.ones(1, 1, Tq, 1, dtype=torch.float64); rw[:, :, active_row] = 0.0
    out["one query row left out of dk / dv"] = (None, rw)
    return out


def _rejected(p, got, dtype="bf16"):
    return [name for name, ratio, where in AC.violations(p, got, dtype) if where is not None]


MUTANT_SHAPES = DEMO + [(1, 2, 600, 333, 1), (2, 4, 77, 150, 1), (1, 2, 33, 129, 1), (1, 1, 513, 65, 2)]


@pytest.mark.parametrize("shape", MUTANT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_budgets_reject_the_mutants(shape):
    """A lost key, a lost tile, a doubled key, a lost query row, another job's dout: each breaks the new bound (bf16, the
    wider one) in some pass of some call of the pointer profile; a lost tile breaks it on the flat profile too."""
    n = AC.n_calls(shape, "pointer")
    hit = {}
    for call in range(n):
        p = AC.problem(shape, "pointer", call)
        row = int(AC.heads(p.dout, shape[1]).abs().sum(-1)[0, 0].nonzero()[0])
        for name, (w, rw) in _mutants(shape, row).items():
            hit.setdefault(name, set()).update(_rejected(p, AC.attend64(p, w=w, rw=rw)))
        other = AC.problem(shape, "pointer", (call + 2) % max(n, 4))
        hit.setdefault("two jobs' dout swapped", set()).update(_rejected(p, AC.attend64(p, dout=other.dout)))
        assert _rejected(p, AC.attend64(p)) == []
    for name, passes in hit.items():
        assert passes, (shape, name)
    assert "o" in hit["last key removed"] and {"dk1", "dv"} <= hit["last key removed"]
    assert {"dk1", "dv"} <= hit["one query row left out of dk / dv"] and "o" not in hit["one query row left out of dk / dv"]
    assert {"dq1", "dk1", "dv"} <= hit["two jobs' dout swapped"]
    p = AC.problem(shape, "flat")
    for name, (w, rw) in _mutants(shape, 0).items():
        if "removed" in name and "last key" not in name:
            assert {"o", "dq1", "dv"} <= set(_rejected(p, AC.attend64(p, w=w))), (shape, name)


# ------------------------------------------------------------------------------------------------ what the Gaussian tests miss
def _gaussian(shape):
    B, H, Tq, S, parts = shape
    E = H * 32
    f = lambda n, seed: rnd((B, n, E), torch.bfloat16, seed).float()
    two = parts == 2
    return AC.Problem(shape, "gaussian", 0, f(Tq, 1), f(S, 2), f(S, 3), f(Tq, 4) if two else None, f(S, 5) if two else None,
                      f(Tq, 6), 0.0, 0, None, None)


def _todays_verdict(shape, w):
    """{pass: accepted?} of the mutant under the inputs and the bound of test_attention_fwd_bwd (bf16: |err| <= 1.6e-2
    (atol scale + |ref|), atol scale 1 for the forward and sqrt(max(Tq, S)) / 2 for the gradients)."""
    p = _gaussian(shape)
    scale = 1.0 / math.sqrt(32 * shape[4])
    ref, got = AC.attend64(p, scale=scale), AC.attend64(p, w=w, scale=scale)
    sc = 0.5 * math.sqrt(max(shape[2], shape[3]))
    return {n: bool(((got[n] - ref[n]).abs() <= 1.6e-2 * ((1.0 if n == "o" else sc) + ref[n].abs())).all())
            for n in ("o", "dq1", "dk1", "dv", "dq2", "dk2")}


def test_todays_bound_accepts_the_same_mutants_at_long_key_sequences():
    """What the new tests add.  On Gaussian operands attention over many keys averages hundreds of small terms: with keys
    removed from the softmax of every pass, the bound of test_attention_fwd_bwd / _attn_run_and_check still accepts all
    five gradients at the cross-attention shape and at the shape whose keys are split across blocks (one lost key: the
    forward too).  The budgets above reject every one of these (test_the_budgets_reject_the_mutants)."""
    grads = ("dq1", "dk1", "dv", "dq2", "dk2")
    for shape in DEMO:
        S = shape[3]
        muts = _mutants(shape, 0)
        for name in ("last key removed", "an aligned run of 32 keys removed", "keys 64..127 removed"):
            verdict = _todays_verdict(shape, muts[name][0])
            assert all(verdict[g] for g in grads), (shape, name, verdict)
            if shape == DEMO[1] and name == "last key removed":
                assert verdict["o"], (shape, name)
            else:
                assert not verdict["o"], (shape, name)
