"""Weight EMA on the device: the table-driven update and swap kernels bit for bit against numpy float32 (every size
around the chunk, aligned and 4-byte-shifted tensors, sentinels around each), the update attached to eager and captured
optimizer steps, evaluation under the average through graphs captured before it was applied, and checkpoints."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if torch.cuda.is_available():
    from future_od.native import lib as L
    from future_od.native import ops
    from test_ema_cpu import ema_weight

SENTINEL = 0x7B3A5C1D                      # a word no update produces: checked before and after every tensor
GUARD = 4                                  # words (one 16-byte access)
SHIFTS = ((0, 0), (1, 0), (0, 1), (1, 1))  # (average, parameter) start this many floats into a 16-byte line


@pytest.fixture(autouse=True)
def _mode_is_restored():
    prev = ops.is_deterministic()
    yield
    ops.set_deterministic(prev)


def _sizes():
    chunk = L.LIB.fod_multi_chunk()
    return [1, 3, 4, 5, 1023, chunk - 1, chunk, chunk + 1, 2 * chunk + 7]


class _Pairs:
    """Every size with every shift, laid out in one buffer per side with sentinel words around each tensor, and the device
    tables of ONE launch over all of them."""

    def __init__(self, seed, odd_words=False):
        rng = np.random.default_rng(seed)
        chunk = L.LIB.fod_multi_chunk()
        self.spans = []                                         # (offset in the average buffer, in the other, n)
        cursor = [0, 0]
        for n in _sizes():
            for shift in SHIFTS:
                at = []
                for side in (0, 1):
                    start = (cursor[side] + 3) // 4 * 4 + GUARD + shift[side]
                    at.append(start)
                    cursor[side] = start + n + GUARD
                self.spans.append((at[0], at[1], n))
        words = [(c + 3) // 4 * 4 + GUARD for c in cursor]
        self.host = [np.full(w, SENTINEL, dtype=np.uint32) for w in words]
        for ea, pa, n in self.spans:
            self.host[0][ea:ea + n] = rng.standard_normal(n).astype(np.float32).view(np.uint32)
            self.host[1][pa:pa + n] = (rng.standard_normal(n) * 3).astype(np.float32).view(np.uint32)
        if odd_words:                                           # words that are not numbers (the swap moves bits)
            odd = np.array([0x7FC00001, 0xFFFFFFFF, 0x00000001, 0x80000000, 0x7F800000], dtype=np.uint32)
            for ea, pa, n in self.spans[-8:]:
                self.host[0][ea:ea + 5] = odd
                self.host[1][pa + n - 5:pa + n] = odd[::-1]
        self.dev = [torch.from_numpy(h.view(np.int32).copy()).to(DEV) for h in self.host]
        assert all(d.data_ptr() % 16 == 0 for d in self.dev)
        base = [d.data_ptr() for d in self.dev]
        pairs = [[base[0] + 4 * ea, base[1] + 4 * pa] for ea, pa, _ in self.spans]
        assert {(a % 16, b % 16) for a, b in pairs} == {(4 * s, 4 * t) for s, t in SHIFTS}
        bt, bc = [], []
        for t, (_, _, n) in enumerate(self.spans):
            for c in range((n + chunk - 1) // chunk):
                bt.append(t)
                bc.append(c)
        self.tab = (torch.tensor(pairs, dtype=torch.int64, device=DEV),
                    torch.tensor([n for _, _, n in self.spans], dtype=torch.int64, device=DEV),
                    torch.tensor(bt, dtype=torch.int32, device=DEV), torch.tensor(bc, dtype=torch.int32, device=DEV))
        self.nblocks = len(bt)

    def args(self):
        return tuple(ops.ptr(t) for t in self.tab) + (self.nblocks,)

    def read(self):
        torch.cuda.synchronize()
        return [d.cpu().numpy().view(np.uint32) for d in self.dev]


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("u", [1, 2, 10, 100000])
def test_update_kernel_is_the_float32_restatement(u, warmup):
    decay = 0.9998
    w = ema_weight(u, decay, warmup)
    if warmup and u == 1:
        assert w == np.float32(9.0 / 11.0)
    pr = _Pairs(seed=u)
    count = torch.tensor([u], dtype=torch.int64, device=DEV)    # the weight comes from this, not from the host
    L.call("fod_multi_ema", *pr.args(), ops.ptr(count), decay, int(warmup), ops.stream())
    got = pr.read()
    want = [h.copy() for h in pr.host]
    for ea, pa, n in pr.spans:
        e, p = pr.host[0][ea:ea + n].view(np.float32), pr.host[1][pa:pa + n].view(np.float32)
        diff = (p - e).astype(np.float32)
        move = (w * diff).astype(np.float32)
        want[0][ea:ea + n] = (e + move).astype(np.float32).view(np.uint32)
    assert np.array_equal(got[1], pr.host[1])                    # the parameters and their sentinels: not written
    bad = np.nonzero(got[0] != want[0])[0]
    assert bad.size == 0, (bad[:8], got[0][bad[:8]], want[0][bad[:8]])
    assert int(count.item()) == u
    assert len(pr.spans) == 36
    for ea, _, n in pr.spans:                                    # every pair was reached
        assert n < 5 or not np.array_equal(got[0][ea:ea + n], pr.host[0][ea:ea + n]), (ea, n)


def test_swap_kernel_exchanges_bits_and_twice_is_the_identity():
    pr = _Pairs(seed=77, odd_words=True)
    L.call("fod_multi_swap", *pr.args(), ops.stream())
    got = pr.read()
    want = [h.copy() for h in pr.host]
    for ea, pa, n in pr.spans:
        want[0][ea:ea + n] = pr.host[1][pa:pa + n]
        want[1][pa:pa + n] = pr.host[0][ea:ea + n]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])      # contents exchanged, sentinels intact
    L.call("fod_multi_swap", *pr.args(), ops.stream())
    back = pr.read()
    assert np.array_equal(back[0], pr.host[0]) and np.array_equal(back[1], pr.host[1])


# ---- the model -----------------------------------------------------------------------------------------------------
def _params(model):
    return [p.detach().clone() for p in model.parameters() if p.requires_grad]


def _advance(avg, params, u, ema):
    """One update of the float32 restatement, each operation a rounding of its own: avg <- avg + w * (p - avg)."""
    w = float(ema_weight(u, ema.decay, ema.warmup))
    return [a + (p - a) * w for a, p in zip(avg, params)]


def _assert_average(ema, want):
    got = [t for _, t in ema.named_tensors()]
    assert len(got) == len(want)
    for (name, _), g, w in zip(ema.named_tensors(), got, want):
        assert torch.equal(g, w), (name, float((g - w).abs().max()))


def _batches():
    from future_od.datasets.synthetic import make_batch
    return (make_batch(2, 3, 96, 128, seed=11, max_boxes=9, device=DEV),
            make_batch(2, 3, 96, 128, seed=12, max_boxes=20, device=DEV))       # other targets, one signature


def test_attached_to_eager_steps_it_follows_and_does_not_touch_training():
    from future_od.optim import WeightEMA
    from test_graph_gpu import _build, _eager_step
    ops.set_deterministic(True)
    data, data2 = _batches()
    m_a, o_a = _build("bf16")
    m_b, o_b = _build("bf16")
    ema = WeightEMA(m_b, decay=0.9998, warmup=True)
    o_b.attach_ema(ema)
    assert ema.num_updates == 0
    names = [n for n, p in m_b.named_parameters() if p.requires_grad]
    assert [n for n, _ in ema.named_tensors()] == names
    for (_, e), p in zip(ema.named_tensors(), (p for p in m_b.parameters() if p.requires_grad)):
        assert e.stride() == p.stride() and e.data_ptr() != p.data_ptr() and e.dtype == torch.float32
    want = _params(m_b)
    _assert_average(ema, want)
    for k, d in enumerate((data, data2, data), start=1):
        _eager_step(m_a, o_a, d)
        _eager_step(m_b, o_b, d)
        want = _advance(want, _params(m_b), k, ema)
        _assert_average(ema, want)
    for (n, pa), (_, pb) in zip(m_a.named_parameters(), m_b.named_parameters()):
        assert torch.equal(pa, pb), n
    assert ema.num_updates == 3 == o_b._step_no


@pytest.mark.parametrize("rollback", [True, False])
def test_captured_step_carries_the_update(rollback):
    from future_od.graph import GraphedStep
    from future_od.optim import WeightEMA
    from test_graph_gpu import _build
    data, data2 = _batches()
    model, opt = _build("bf16")
    ema = WeightEMA(model)
    opt.attach_ema(ema)
    step = GraphedStep(model, opt, warmup=2, rollback_warmup=rollback)
    want = _params(model)
    step(data)
    if rollback:
        # the warm-up steps were put back, the average and its count with them: one update, from the initial weights
        assert ema.num_updates == opt._step_no == 1
        want = _advance(want, _params(model), 1, ema)
        _assert_average(ema, want)
    else:
        # two warm-up steps, one through the device-side step count and the replay: four real steps
        assert ema.num_updates == opt._step_no == 4
        want = [t.clone() for _, t in ema.named_tensors()]
    first = opt._step_no
    for k, d in enumerate((data2, data, data2), start=1):
        step(d)
        assert ema.num_updates == opt._step_no == first + k
        want = _advance(want, _params(model), first + k, ema)
        _assert_average(ema, want)
    assert step.replays == 4 and len(step._graphs) == 1
    (g,) = step._graphs.values()
    assert g["record"].of("weight ema")                          # the graph keeps the tables and tensors it reads


def _same(a, b):
    return set(a) == set(b) == {"scores", "labels", "boxes", "query", "count"} and all(torch.equal(a[k], b[k]) for k in a)


def _clone(det):
    return {k: v.clone() for k, v in det.items()}


def test_evaluating_under_the_average():
    from future_od.graph import GraphedPredict, GraphedStep
    from future_od.optim import WeightEMA
    from test_graph_gpu import _build, _eager_step
    data, data2 = _batches()
    free = {k: v for k, v in data.items()
            if k not in ("boxes", "classes", "active", "ignore_boxes", "annotated_frame_idx", "_host_annotations")}
    model, opt = _build("bf16")
    ema = WeightEMA(model, decay=0.5, warmup=False)              # a short memory: three steps move the average visibly
    opt.attach_ema(ema)
    for d in (data, data2, data):
        _eager_step(model, opt, d)
    # the reference result first: a second model built fresh and loaded with the averaged state (build_model starts a
    # new prepared-operand store, so a graph of `model` is captured after it, not before)
    other, _ = _build("bf16", seed=4)
    other.load_state_dict(ema.model_state_dict())
    want = _clone(other.predict(free, top_k=50))
    gp = GraphedPredict(model, top_k=50)                         # captured BEFORE the average is applied
    raw_graph, raw_eager = _clone(gp(free)), _clone(model.predict(free, top_k=50))
    assert _same(raw_graph, raw_eager) and not _same(want, raw_eager)
    before = _params(model)
    average = [t.clone() for _, t in ema.named_tensors()]
    with ema.applied():
        assert ema.is_applied
        assert _same(_clone(gp(free)), want) and _same(model.predict(free, top_k=50), want)
        for p, a in zip((p for p in model.parameters() if p.requires_grad), average):
            assert torch.equal(p, a)
        sd = model.state_dict()
        assert all(torch.equal(sd[n], a) for (n, _), a in zip(ema.named_tensors(), average))
        with pytest.raises(RuntimeError, match="applied"):
            opt.step()
        with pytest.raises(RuntimeError, match="applied"):
            GraphedStep(model, opt)(data)
        with pytest.raises(RuntimeError, match="nest"):
            with ema.applied():
                pass
    assert not ema.is_applied and len(gp._graphs) == 1
    assert _same(_clone(gp(free)), raw_graph) and _same(model.predict(free, top_k=50), raw_eager)
    for p, b in zip((p for p in model.parameters() if p.requires_grad), before):
        assert torch.equal(p, b)
    _assert_average(ema, average)
    assert ema.num_updates == 3 == opt._step_no                  # nothing inside counted as a step


class _Loader(list):
    batch_size = 2


def test_checkpoints_carry_the_average(tmp_path):
    from future_od.datasets.synthetic import make_batch
    from future_od.models.st_detr import SpatioTemporalDETRArgs
    from future_od.optim import WeightEMA
    from future_od.trainer import Trainer
    from runs._helper import get_lr_func, setup_optimizer
    from runs._model import build_model
    from test_graph_gpu import _eager_step
    torch.manual_seed(0)
    args = SimpleNamespace(device=DEV, distributed=False, compute_dtype="bf16", backbone="resnet18")
    detr = SpatioTemporalDETRArgs(num_classes=8, num_queries=32, lr_backbone=1e-4, enc_layers=1, dec_layers=2,
                                  pretrained_backbone=False)
    batch = make_batch(2, 3, 96, 128, seed=1, max_boxes=5, device=DEV)

    def trainer(name, with_ema=True):
        model = build_model(args, detr)
        sched, opt = setup_optimizer(detr, model, get_lr_func(4))
        ema = WeightEMA(model, decay=0.9) if with_ema else None
        tr = Trainer(model, opt, sched, _Loader([batch]), {"val": _Loader([batch])}, str(tmp_path), str(tmp_path), name,
                     DEV, print_interval=3, visualization_epochs=[], visualization_iterations=[], category_dict={},
                     checkpoint_epochs=True, is_master=True, max_norm=detr.max_norm, ema=ema)
        return model, opt, ema, tr

    model, opt, ema, tr = trainer("t")
    assert opt._ema is ema
    model.eval()
    for _ in range(2):
        _eager_step(model, opt, batch)
    assert ema.num_updates == 2
    tr.save_checkpoint(is_final=True)
    ck = torch.load(tmp_path / "t.pth.tar", map_location="cpu", weights_only=False)
    assert set(ck["ema"]) == {"decay", "warmup", "num_updates", "params"} and ck["ema"]["num_updates"] == 2
    # round trip: tensors and count
    model2, _, ema2, tr2 = trainer("t")
    where = [t.data_ptr() for _, t in ema2.named_tensors()]
    tr2.load_checkpoint()
    assert ema2.num_updates == 2 and [t.data_ptr() for _, t in ema2.named_tensors()] == where
    _assert_average(ema2, [t for _, t in ema.named_tensors()])
    assert not all(torch.equal(t, p) for (_, t), p in zip(ema2.named_tensors(), _params(model2)))
    # a file without an average: started again from the loaded weights
    ck.pop("ema")
    torch.save(ck, tmp_path / "plain.pth.tar")
    tr2.load_checkpoint(str(tmp_path / "plain.pth.tar"))
    assert ema2.num_updates == 0
    _assert_average(ema2, _params(model2))
    # a file with an average loads into a trainer without one
    model3, _, _, tr3 = trainer("t", with_ema=False)
    tr3.load_checkpoint()
    assert all(torch.equal(v, model3.state_dict()[k]) for k, v in model.state_dict().items())
    # the final file: the averaged weights as a state dict of the model
    final = torch.load(tmp_path / "t_final.pth.tar", map_location="cpu", weights_only=False)
    assert set(final) == {"net", "net_ema"} and list(final["net_ema"]) == list(final["net"])
    model3.load_state_dict(final["net_ema"])
    got = dict(model3.named_parameters())
    assert all(torch.equal(got[n], t) for n, t in ema.named_tensors())
