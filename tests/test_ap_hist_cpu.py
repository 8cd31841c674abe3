"""Streaming AP, the parts that need no GPU: ops.ap_hist_accum / ap_hist_finalize on CPU tensors against the numpy
restatement of tests/ap_hist_cases.py (integers, pr, pr_score and NaN positions byte for byte; ap and ap101 within
(n + 3) * 2^-53), the hand example against literals, the tie to the sorted AP where no bin is shared, both producers' one
score for every threshold, StreamingDetectionEvaluator (two gloo ranks included), the trainer's switch, and the two entry
points as the binding reads them from include/fod_ext.h with their refusals (they return before any launch)."""
import inspect
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ap_hist_cases as AC
from future_od.native import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, LONG = "pointer", "int", "long"
ACCUM, FINALIZE = "fod_ap_hist_accum", "fod_ap_hist_finalize"
CASES = AC.all_cases()
IDS = [c["name"] for c in CASES]
UNIQUE = [c for c in CASES if c["name"].startswith("unique")]
U = 2.0 ** -53


def _od(batch):
    return tuple(torch.from_numpy(a.copy()) for a in batch)


def _accumulate(case, batches=None):
    from future_od.native import ops
    state = ops.ap_hist_state(case["T"], case["C1"], "cpu")
    for b in case["batches"] if batches is None else batches:
        assert ops.ap_hist_accum(_od(b), state) is state
    return state


# ---- the CPU form against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cpu_form_equals_the_restatement(case):
    from future_od.native import ops
    state = _accumulate(case)
    before = [t.clone() for t in state]
    outs = ops.ap_hist_finalize(state)
    assert all(torch.equal(a, b) for a, b in zip(state, before))                 # finalise reads the state only
    AC.assert_results([t.numpy() for t in state], [t.numpy() for t in outs], case, "cpu form")
    # one batch after the other == their concatenation; and the order of the batches does not matter
    for other in ([AC.concatenated(case)], case["batches"][::-1]):
        for a, b in zip(_accumulate(case, other), state):
            assert torch.equal(a, b)


def test_cases_cover_what_they_claim():
    sizes = {b[0].shape[2] for c in CASES for b in c["batches"]}
    assert {1, 63, 64, 65, 257, 1000} <= sizes
    assert {(c["T"]) for c in CASES} >= {1, 10, 16} and {c["C1"] for c in CASES} >= {2, 10}
    assert any(len(c["batches"]) == 3 for c in CASES)
    placed = next(c for c in CASES if c["name"].startswith("placed"))
    tp, seen, anno, ap = placed["want"][0], placed["want"][1], placed["want"][2], placed["want"][3]
    keys = set(np.flatnonzero(seen[0, 0]).tolist())
    edges = {k for k in range(AC.WAVE, AC.NB, AC.WAVE)}
    assert {0, AC.TOP} <= keys and all({k - 1, k} <= keys for k in edges) and AC.CHUNK % AC.WAVE == 0
    assert seen[1, 0].sum() > 0 and tp[:, 1].sum() == 0 and anno[1, 0] > 0 and (ap[:, 1, 0] == 0).all()      # no true positive
    odd = [AC.key_of(s) for s in AC.ODD_SCORES]
    assert odd[:5] == [0] * 5 and odd[5:8] == [AC.TOP] * 3 and 0 < odd[8] < odd[9] == 0x80 and odd[10] == AC.TOP \
        and odd[11] == AC.TOP - 1
    assert np.flatnonzero(seen[3, 0]).tolist() == [0] and seen[3, 0, 0] == 40 and tp[0, 3, 0, 0] > 0          # lowest bin only
    assert sorted(seen[4, 0][seen[4, 0] > 0].tolist()) == [300, 300]                                          # one bin, many
    assert anno[5, 0] == 0 and seen[5, 0].sum() == 30 and np.isnan(ap[:, 5]).all()                            # A == 0
    assert seen[6].sum() == 0 and anno[6, 0] > 0 and (ap[:, 6] == 0).all()
    assert seen[7].sum() == 2 and tp[:, 7].sum() == 2 * placed["T"]                                           # padding adds nothing
    for case in UNIQUE:
        assert not AC.shared_bins(case["batches"], case["C1"]).any(), case["name"]
        assert case["want"][1].max() == 1
    assert any(AC.shared_bins(c["batches"], c["C1"]).any() for c in CASES if c["name"].startswith("random"))


def test_hand_example():
    from future_od.native import ops
    case = AC.hand_case()
    state = _accumulate(case)
    ap, ap101, pr, score, totals = (t.numpy() for t in ops.ap_hist_finalize(state))
    restated = AC.restate_finalize(*AC.restate_accum(case["batches"], 1, 2))
    for got in ((ap, ap101, pr, score, totals), restated):
        assert np.array_equal(got[4], AC.HAND_TOTALS)
        assert np.array_equal(np.isnan(got[0]), np.isnan(AC.HAND_AP)) and np.array_equal(np.isnan(got[1]), np.isnan(AC.HAND_AP))
        assert np.nanmax(np.abs(got[0] - AC.HAND_AP)) <= 6 * U and np.nanmax(np.abs(got[1] - AC.HAND_AP101)) <= 104 * U
        assert got[2][0, 0, 0].tobytes() == AC.HAND_PR_CLASS0_ALL.tobytes()
        assert got[3][0, 0, 0].tobytes() == AC.HAND_SCORE_CLASS0_ALL.tobytes()
        assert (got[2][0, 0, 1] == 1.0).all() and (got[3][0, 0, 1] == 0.75).all()         # one annotation, found first
        assert got[2][0, 0, 2].tolist() == [1.0] * 34 + [0.0] * 67 and np.isnan(got[2][0, :, 3]).all()
        # a row whose only candidate is negative: recall 0 is answered by its bin, with precision 0
        assert got[2][0, 1, 0].tolist() == [0.0] * 101 and got[3][0, 1, 0].tolist() == [0.5] + [0.0] * 100
    assert [AC.key_of(s) for s in (0.75, 0.5, 0.25)] == [0x3F40, 0x3F00, 0x3E80]


def test_keys_are_the_bf16_truncation():
    from future_od.native import ops
    rng = np.random.default_rng(0)
    s = np.concatenate([np.array(AC.ODD_SCORES, np.float32), rng.random(4000).astype(np.float32) ** 4,
                        rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    want = np.array([AC.key_of(x) for x in s])
    assert np.array_equal(ops.ap_hist_keys(torch.from_numpy(s)).numpy(), want)
    inside = (s > 0) & (s < 1)
    assert np.array_equal(want[inside], torch.from_numpy(s[inside]).view(torch.int32).numpy() >> 16)
    assert ops.AP_HIST_BINS == AC.NB == 16257 and AC.edge_of(AC.TOP) == 1.0 and AC.edge_of(0) == 0.0


# ---- the tie to the sorted AP --------------------------------------------------------------------------------------------
def _f32_ap(od):
    from future_od.utils.od_map import _get_ap
    confs, is_pos, sizes, num_annos = (torch.from_numpy(a.copy()) for a in od)
    return torch.stack([_get_ap(confs[t], is_pos[t].bool(), sizes.bool(), num_annos[:, :, None])
                        for t in range(confs.shape[0])]).numpy()


@pytest.mark.parametrize("case", UNIQUE, ids=[c["name"] for c in UNIQUE])
def test_ap_is_the_sorted_ap_where_no_bin_is_shared(case, capsys):
    from future_od.native import ops
    from future_od.utils.od_map import aggregate_mean_average_precision
    od = AC.concatenated(case)
    assert not AC.shared_bins(case["batches"], case["C1"]).any()
    ap = ops.ap_hist_finalize(_accumulate(case))[0].numpy()
    exact = AC.sorted_ap_f64(*od)
    n = AC.nonempty_bins(case["want"][0], case["want"][1])[None]
    assert np.array_equal(np.isnan(ap), np.isnan(exact)) and (~np.isnan(exact)).sum() > exact.size // 2
    err = np.where(np.isnan(exact), 0.0, np.abs(ap - exact))
    assert (err <= (n + 3) * U).all(), (case["name"], err.max())
    # the existing float32 function on the same tensors: held to three times ITS distance to the float64 evaluation
    tensors = tuple(torch.from_numpy(a.copy()) for a in od)
    table = aggregate_mean_average_precision(tensors[0], tensors[1].bool(), tensors[2].bool(), tensors[3][:, :, None], "cpu")
    f32 = torch.cat([table["all"], table["generic"][:, None]], dim=1).numpy()
    assert f32.dtype == np.float32 and np.array_equal(f32, _f32_ap(od), equal_nan=True)
    finite = ~np.isnan(exact) & np.isfinite(f32)
    measured = np.abs(f32.astype(np.float64) - exact)[finite].max()
    recorded = AC.F32_DISTANCE[case["name"]]
    print(f"{case['name']}: float32 AP is {measured:.3e} from the float64 evaluation (recorded {recorded:.3e})")
    assert 0 < measured <= recorded <= 2 * measured, (case["name"], measured, recorded)
    assert np.abs(ap - f32.astype(np.float64))[finite].max() <= 3 * recorded


# ---- both producers write one score for every threshold ------------------------------------------------------------------
def test_detect_od_map_writes_one_score_for_every_threshold():
    import detect_eval_cases as DC
    from future_od.native import ops
    for case in DC.all_cases()[:6]:
        confs = ops.detect_od_map(*(torch.from_numpy(case[k].copy()) for k in DC.ROWS + DC.ANNOS), case["imsize"],
                                  case["C"], case["per_class"], T=case["T"])[0]
        assert all(confs[t].numpy().tobytes() == confs[0].numpy().tobytes() for t in range(confs.shape[0]))
        want = case["want"][0]                               # ... and so does the definition the kernel is tested against
        assert all(want[t].tobytes() == want[0].tobytes() for t in range(want.shape[0]))


def test_od_map_oracle_writes_one_score_for_every_threshold():
    import detect_eval_cases as DC
    from oracle import od_map as OM
    case = next(c for c in DC.all_cases() if c["name"].startswith("all-pairs"))
    confs = OM.prepare_od_map_stuffs(case["px"], case["dense"], case["anno_boxes"], case["anno_classes"],
                                     case["anno_active"], case["imsize"])[0]
    assert all(confs[t].tobytes() == confs[0].tobytes() for t in range(confs.shape[0]))


# ---- the evaluator ---------------------------------------------------------------------------------------------------------
EV_C = 7                                   # classes of the evaluator tests: 32 (class, size) rows


def _evaluator_batches(seeds=(21, 22, 23, 24), K=16, C=EV_C, N=6):
    """Detection rows and annotations as `predict` and the loaders hand them over, on the host.  The scores of all batches
    are drawn from the bins without replacement except for ONE pair, so exactly the rows of that pair share a bin."""
    out, B = [], 2
    keys = torch.randperm(AC.NB - 1, generator=torch.Generator().manual_seed(20))[:len(seeds) * B * K] + 1
    keys[-1] = keys[0]
    for i, seed in enumerate(seeds):
        g = torch.Generator().manual_seed(seed)
        xy = torch.rand(B, K, 2, generator=g) * torch.tensor([96.0, 64.0])
        wh = torch.rand(B, K, 2, generator=g) * 30 + 2
        boxes = torch.cat([xy, xy + wh], dim=2)
        low = torch.randint(0, 1 << 16, (B, K), generator=g)
        scores = ((keys[i * B * K:(i + 1) * B * K].view(B, K) << 16) | low).to(torch.int32).view(torch.float32)
        scores = scores.sort(dim=1, descending=True).values
        det = {"scores": scores, "labels": torch.randint(0, C, (B, K), generator=g, dtype=torch.int32), "boxes": boxes,
               "query": torch.randint(0, 12, (B, K), generator=g, dtype=torch.int32),
               "count": torch.tensor([K, K - 5], dtype=torch.int32)}
        pick = torch.randint(0, K, (B, N), generator=g)
        anno = boxes.gather(1, pick[:, :, None].expand(-1, -1, 4)) + torch.rand(B, N, 4, generator=g) * 3
        data = {"boxes": anno, "classes": det["labels"].gather(1, pick).long(),
                "active": (torch.rand(B, N, generator=g) < 0.8).long(), "video": torch.zeros(B, 1, 3, 64, 96)}
        out.append((det, data))
    return out


def _bytes(res):
    """Every tensor and array of an evaluator's dict, by name."""
    flat = {}
    for k, v in res.items():
        for k2, v2 in (v.items() if isinstance(v, dict) else [("", v)]):
            flat[k + "/" + k2] = (v2.numpy() if isinstance(v2, torch.Tensor) else np.asarray(v2)).tobytes()
    return flat


def test_streaming_evaluator_on_the_host():
    from future_od.utils.od_map import DetectionEvaluator, StreamingDetectionEvaluator, aggregate_mean_average_precision
    batches = _evaluator_batches()
    kept, stream = DetectionEvaluator(EV_C), StreamingDetectionEvaluator(EV_C)
    for det, data in batches:
        kept.update(det, data)
        stream.update(det, data)
    assert len(stream) == len(kept) == 4 and len(stream._bufs) == 1
    with pytest.raises(RuntimeError, match="no per-batch tensors"):
        stream.tensors()
    with pytest.raises(ValueError, match="box_map"):
        stream.update(dict(batches[0][0], box_map=torch.eye(3)), batches[0][1])
    want, got = kept.aggregate("cpu"), stream.aggregate("cpu")
    assert set(got) == set(want) | {"coco", "pr_curve"} and set(got["coco"]) == set(want) - {"operating_point"}
    assert set(got["pr_curve"]) == {"precision", "score", "recall"} and got["pr_curve"]["recall"][50] == 0.5
    assert got["pr_curve"]["precision"].shape == (10, EV_C + 1, 4, 101) and got["all"].shape == want["all"].shape == (10, EV_C, 4)
    for k in ("detections", "true_positives", "annotations", "precision", "recall", "f1"):       # equal integers, so equal ratios
        assert got["operating_point"][k].numpy().tobytes() == want["operating_point"][k].numpy().tobytes(), k
    # the reference side with its scores truncated to bf16: rows in which a bin is shared are named and left out
    confs, is_pos, sizes, num_annos = (t.numpy() for t in kept.tensors())
    trunc = (confs.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    od = (trunc, is_pos.view(np.uint8), sizes.view(np.uint8), num_annos.sum(axis=2))
    shared = AC.shared_bins([od], EV_C + 1)
    print("rows (class, size) that share a bin:", np.argwhere(shared).tolist())
    assert 0 < shared.sum() and shared.sum() * 10 <= shared.size      # the cap: at most a tenth of the rows
    exact = AC.sorted_ap_f64(*od)
    ap = torch.cat([got["all"], got["generic"][:, None]], dim=1).numpy()
    keep = ~shared[None] & ~np.isnan(exact)
    assert np.array_equal(np.isnan(ap), np.isnan(exact)) and keep.sum() > keep.size // 2
    n = (trunc[0] > 0).sum(axis=1).max()                     # no row has more bins than its class has slots
    assert np.abs(ap - exact)[keep].max() <= (n + 3) * U
    f32 = aggregate_mean_average_precision(torch.from_numpy(trunc), *kept.tensors()[1:], "cpu")
    f32 = torch.cat([f32["all"], f32["generic"][:, None]], dim=1).numpy().astype(np.float64)
    assert np.abs(ap - f32)[keep].max() <= 3 * np.abs(f32 - exact)[keep].max()
    assert ((got["coco"]["all"].numpy() >= 0) | np.isnan(got["coco"]["all"].numpy())).all()
    # reset zeroes the state in place; a second pass gives the same bytes
    first, state = _bytes(got), stream.state()
    stream.reset()
    assert len(stream) == 0 and stream.state() is state and all(int(t.abs().sum()) == 0 for t in state)
    for det, data in batches[::-1]:
        stream.update(det, data)
    assert _bytes(stream.aggregate()) == first
    # the dense path's four tensors go in just as well
    dense = StreamingDetectionEvaluator(EV_C)
    for i in range(len(kept)):
        dense.update_od(tuple(kept._od[k][i] for k in range(4)))
    assert all(torch.equal(a, b) for a, b in zip(dense.state(), stream.state()))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from future_od.utils.od_map import StreamingDetectionEvaluator
    ev = StreamingDetectionEvaluator(EV_C)
    for det, data in _evaluator_batches()[rank::world]:
        ev.update(det, data)
    res = _bytes(ev.aggregate())
    again = _bytes(ev.aggregate())                           # the local state was not overwritten by the sum
    q.put((rank, res, again == res, len(ev)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_return_the_bytes_of_one_process():
    from future_od.utils.od_map import StreamingDetectionEvaluator
    one = StreamingDetectionEvaluator(EV_C)
    for det, data in _evaluator_batches():
        one.update(det, data)
    want = _bytes(one.aggregate())
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, got, stable, updates in res:
        assert updates == 2 and stable and set(got) == set(want)
        assert all(got[k] == want[k] for k in want), (rank, [k for k in want if got[k] != want[k]])


def test_trainer_accepts_more_than_one_rank_only_when_streaming(monkeypatch):
    from future_od.trainer import Trainer
    tr = Trainer.__new__(Trainer)
    tr._distributed = True
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError, match="ranks"):
        tr.evaluate_detections()
    assert tr.set_streaming_evaluation() is tr and tr._streaming_eval
    with pytest.raises(AttributeError):                      # past the refusal: this bare object has no model to run
        tr.evaluate_detections()
    tr.set_streaming_evaluation(False)
    with pytest.raises(NotImplementedError, match="ranks"):
        tr.evaluate_detections()


def test_existing_signatures_did_not_move():
    from future_od.trainer import Trainer
    from future_od.utils import od_map
    sig = inspect.signature(Trainer.evaluate_detections).parameters
    assert list(sig) == ["self", "top_k", "score_threshold", "per_query", "nms", "nms_class_agnostic", "per_class"]
    assert list(inspect.signature(od_map.DetectionEvaluator.__init__).parameters) == ["self", "num_classes", "per_class"]
    assert list(inspect.signature(od_map.StreamingDetectionEvaluator.__init__).parameters) == ["self", "num_classes", "per_class"]
    assert list(inspect.signature(od_map.aggregate_mean_average_precision).parameters) == \
        ["confs", "is_positive", "size_categories", "num_annos", "device"]


# ---- ABI and binding -------------------------------------------------------------------------------------------------------
def test_entries_are_bound_with_the_headers_signatures_and_the_abi_moved():
    from future_od.native import lib as L
    hdr = open(os.path.join(ROOT, "include", "fod.h")).read()
    assert int(re.search(r"#define FOD_ABI_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == L.LIB.fod_abi_version() >= 20
    assert abi.EXT_PROTOTYPES[ACCUM] == (I, [P] * 4 + [I, I, LONG] + [P] * 4)
    assert abi.EXT_PROTOTYPES[FINALIZE] == (I, [P] * 3 + [I, I] + [P] * 6)
    for entry in (ACCUM, FINALIZE):
        assert entry not in abi.PROTOTYPES and entry not in hdr and entry in L.EXT_SIGNATURES
        fn = getattr(L.LIB, entry)
        assert fn.restype is abi.CTYPE[I] and list(fn.argtypes) == [abi.CTYPE[k] for k in abi.EXT_PROTOTYPES[entry][1]]
    assert "ap_hist" in open(os.path.join(ROOT, "future-object-detection_amd", "build.sh")).read()


def _accum(T=10, C1=3, P_=5, null=()):
    """The non-null 'pointers' are the address 8: a launch would fault, so a clean non-zero return is the check itself."""
    from future_od.native import lib as L
    p = [None if k in null else 8 for k in range(7)]
    rc = getattr(L.LIB, ACCUM)(*p[:4], T, C1, P_, *p[4:], None)
    return rc, L.last_error()


def _finalize(T=10, C1=3, null=()):
    from future_od.native import lib as L
    p = [None if k in null else 8 for k in range(8)]
    rc = getattr(L.LIB, FINALIZE)(*p[:3], T, C1, *p[3:], None)
    return rc, L.last_error()


@pytest.mark.parametrize("entry, kw, texts", [
    (_accum, dict(T=0), ("T=0", "1..16")), (_accum, dict(T=17), ("T=17", "1..16")), (_accum, dict(T=-1), ("T=-1", "1..16")),
    (_accum, dict(C1=1), ("C1=1", "at least 2")), (_accum, dict(C1=0), ("C1=0", "at least 2")),
    (_accum, dict(P_=0), ("P_total=0", "at least 1")), (_accum, dict(P_=-3), ("P_total=-3", "at least 1")),
    (_accum, dict(C1=1 << 20, P_=1 << 40), ("workgroups",)),
    (_finalize, dict(T=0), ("T=0", "1..16")), (_finalize, dict(T=17), ("T=17", "1..16")),
    (_finalize, dict(C1=1), ("C1=1", "at least 2")), (_finalize, dict(C1=-1), ("C1=-1", "at least 2")),
] + [(_accum, dict(null=(k,)), ("null operand",)) for k in range(7)]
  + [(_finalize, dict(null=(k,)), ("null operand",)) for k in range(8)])
def test_arguments_are_refused_before_any_launch(entry, kw, texts):
    from future_od.native import lib as L
    rc, err = entry(**kw)
    who = "ap_hist_accum:" if entry is _accum else "ap_hist_finalize:"
    assert rc == L.ERR_ARG and err.startswith(who) and all(t in err for t in texts), (kw, rc, err)


def test_wrappers_refuse_bad_operands():
    from future_od.native import lib as L
    from future_od.native import ops
    confs, is_pos, sizes, num_annos = _od(AC.hand_case()["batches"][0])
    state = ops.ap_hist_state(1, 2, "cpu")
    run = lambda od, st=state: (lambda: ops.ap_hist_accum(od, st))
    for bad in (run((confs.double(), is_pos, sizes, num_annos)), run((confs, is_pos.int(), sizes, num_annos)),
                run((confs, is_pos, sizes[:, :3], num_annos)), run((confs, is_pos, sizes, num_annos.int())),
                run((confs[:, :, :3], is_pos, sizes, num_annos)), run((confs, is_pos, sizes)),
                run((confs.transpose(1, 2).contiguous().transpose(1, 2), is_pos, sizes, num_annos)),
                run((confs, is_pos, sizes, num_annos), ops.ap_hist_state(2, 2, "cpu")),
                run((confs, is_pos, sizes, num_annos), (state[0].long(), state[1], state[2])),
                run((confs, is_pos, sizes, num_annos), state[:2]),
                lambda: ops.ap_hist_finalize((state[0], state[1][:, :, :5], state[2])),
                lambda: ops.ap_hist_state(0, 2, "cpu"), lambda: ops.ap_hist_state(17, 2, "cpu"),
                lambda: ops.ap_hist_state(1, 1, "cpu")):
        with pytest.raises(L.FodError, match="ap_hist"):
            bad()
    assert int(state[1].sum()) == 0                          # nothing was added on the way
    ops.ap_hist_accum((confs, is_pos.bool(), sizes.bool(), num_annos), state)      # bool flags are taken as well
    assert int(state[1].sum()) == 7
