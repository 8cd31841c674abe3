"""Gradient accumulation on the device: the table-driven kernel bit for bit against the same float32 operations done by
torch on the host (every size around the chunk, 16-byte-aligned and 4-byte-shifted tensors, sentinels around each), and
the captured step with `accumulate=N` -- the accumulated gradient, the one optimizer step per cycle, the cycle's
bookkeeping, dropout, two data-parallel ranks and the Trainer's two loops."""
import functools
import os
import socket
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
    from future_od.native import functional as Fn
    from future_od.native import lib as L
    from future_od.native import ops

SENTINEL = 0x7B3A5C1D                      # a word none of the modes produces: checked around every tensor
GUARD = 4                                  # words (one 16-byte access)
SHIFTS = ((0, 0), (0, 1), (1, 0))          # (accumulator, gradient) start this many floats into a 16-byte line
STORE, ADD, FINISH = 0, 1, 2


@pytest.fixture(autouse=True)
def _mode_is_restored():
    prev = ops.is_deterministic()
    yield
    ops.set_deterministic(prev)


# ---- the kernel through the C ABI ------------------------------------------------------------------------------------
def _values(n, gen):
    """Normal-range values, both signs: |x| log-uniform in [1e-3, 1e3] -- sums and products stay far from subnormals."""
    mag = torch.pow(10.0, torch.rand(n, generator=gen, dtype=torch.float64) * 6.0 - 3.0)
    sign = torch.randint(0, 2, (n,), generator=gen, dtype=torch.float64) * 2.0 - 1.0
    return (mag * sign).to(torch.float32)


@functools.lru_cache(maxsize=None)
def _layout():
    """Every size with every alignment, laid out in one host buffer per side (accumulator, gradient) with sentinel words
    around each tensor, and the host tables of ONE launch over all of them.  Built once, never written."""
    chunk = L.LIB.fod_multi_chunk()
    assert chunk == 16384
    sizes = [1, 3, 4, 5, 1023, 1025, chunk - 1, chunk, chunk + 1, 2 * chunk + 7]
    gen = torch.Generator().manual_seed(20)
    spans, cursor = [], [0, 0]                                   # (offset in the accumulator buffer, in the other, n)
    for n in sizes:
        for shift in SHIFTS:
            at = []
            for side in (0, 1):
                start = (cursor[side] + 3) // 4 * 4 + GUARD + shift[side]
                at.append(start)
                cursor[side] = start + n + GUARD
            spans.append((at[0], at[1], n))
    host = [torch.full(((c + 3) // 4 * 4 + GUARD,), SENTINEL, dtype=torch.int32) for c in cursor]
    for aa, ga, n in spans:
        host[0][aa:aa + n] = _values(n, gen).view(torch.int32)
        host[1][ga:ga + n] = _values(n, gen).view(torch.int32)
    bt, bc = [], []
    for t, (_, _, n) in enumerate(spans):
        for c in range((n + chunk - 1) // chunk):
            bt.append(t)
            bc.append(c)
    assert len(spans) == 30 and len(bt) == 30 + 3 * (1 + 2)      # C + 1 takes two blocks, 2C + 7 three
    return spans, host, bt, bc


def _launch(mode, scale):
    """One launch of `mode` over fresh device copies of the layout; returns the two buffers as they are afterwards."""
    spans, host, bt, bc = _layout()
    dev = [h.to(DEV) for h in host]
    assert all(d.data_ptr() % 16 == 0 for d in dev)
    pairs = [[dev[0].data_ptr() + 4 * aa, dev[1].data_ptr() + 4 * ga] for aa, ga, _ in spans]
    assert {(a % 16, g % 16) for a, g in pairs} == {(4 * s, 4 * t) for s, t in SHIFTS}
    tab = (torch.tensor(pairs, dtype=torch.int64, device=DEV),
           torch.tensor([n for _, _, n in spans], dtype=torch.int64, device=DEV),
           torch.tensor(bt, dtype=torch.int32, device=DEV), torch.tensor(bc, dtype=torch.int32, device=DEV))
    L.call("fod_multi_accum", *(ops.ptr(t) for t in tab), len(bt), mode, scale, ops.stream())
    torch.cuda.synchronize()
    return [d.cpu() for d in dev]


def _assert_words(got, want, what):
    bad = torch.nonzero(got != want).flatten()
    assert bad.numel() == 0, (what, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def test_store_moves_the_gradient_and_leaves_it():
    spans, host, _, _ = _layout()
    got = _launch(STORE, 1.0)
    want = host[0].clone()
    for aa, ga, n in spans:
        want[aa:aa + n] = host[1][ga:ga + n]
    _assert_words(got[0], want, "accumulator")                   # acc == g, sentinels intact
    _assert_words(got[1], host[1], "gradient")                   # g and its sentinels: not written


def test_add_is_the_float32_sum():
    spans, host, _, _ = _layout()
    got = _launch(ADD, 1.0)
    want = host[0].clone()
    for aa, ga, n in spans:
        a, g = host[0][aa:aa + n].view(torch.float32), host[1][ga:ga + n].view(torch.float32)
        want[aa:aa + n] = (a + g).view(torch.int32)
    _assert_words(got[0], want, "accumulator")
    _assert_words(got[1], host[1], "gradient")
    for aa, _, n in spans:                                       # every pair was reached
        assert not torch.equal(got[0][aa:aa + n], host[0][aa:aa + n]), (aa, n)


def test_finish_is_the_float32_sum_times_the_float32_scale():
    spans, host, _, _ = _layout()
    scale = torch.tensor(1.0 / 3.0, dtype=torch.float32)
    got = _launch(FINISH, float(scale))
    want = host[1].clone()
    for aa, ga, n in spans:
        a, g = host[0][aa:aa + n].view(torch.float32), host[1][ga:ga + n].view(torch.float32)
        want[ga:ga + n] = ((a + g) * scale).view(torch.int32)    # the sum rounded, then the product rounded
    _assert_words(got[1], want, "gradient")
    _assert_words(got[0], host[0], "accumulator")                # acc and its sentinels: not written
    for _, ga, n in spans:
        assert not torch.equal(got[1][ga:ga + n], host[1][ga:ga + n]), (ga, n)


def test_accumulator_object_runs_a_cycle_and_follows_moved_tensors():
    """GradAccumulator over three tensors (one of them a 4-byte-shifted view): store, add, finish(3) give
    ((g1 + g2) + g3) * float32(1/3); rebind() points it at clones at other addresses, what was accumulated stays."""
    from future_od.optim import GradAccumulator
    gen = torch.Generator().manual_seed(3)
    sizes = (5, 16384 + 9, 1000)
    host = [[_values(n, gen) for n in sizes] for _ in range(3)]              # three micro-batches' gradients
    back = torch.zeros(1001, device=DEV)
    grads = [torch.empty(5, device=DEV), torch.empty(16384 + 9, device=DEV), back[1:]]
    acc = GradAccumulator(grads)
    assert acc.numel == sum(sizes) and acc.nbytes >= 4 * sum(sizes) and not acc.moved(grads)
    for g, h in zip(grads, host[0]):
        g.copy_(h)
    acc.store()
    for g, h in zip(grads, host[1]):
        g.copy_(h)
    acc.add()
    for a, h1, h2 in zip(acc.accumulated(), host[0], host[1]):
        assert torch.equal(a.cpu(), h1 + h2)
    moved = [torch.empty_like(g) for g in grads]
    assert acc.moved(moved)
    acc.rebind(moved)
    for g, h in zip(moved, host[2]):
        g.copy_(h)
    acc.finish(3)
    third = torch.tensor(1.0 / 3.0, dtype=torch.float32)
    for g, old, h1, h2, h3 in zip(moved, grads, *host):
        assert torch.equal(g.cpu(), ((h1 + h2) + h3) * third)
        assert torch.equal(old.cpu(), h2)                                    # the old addresses: no longer written
    with pytest.raises(L.FodError, match="sizes"):
        acc.rebind(moved[:2] + [torch.empty(7, device=DEV)])


# ---- the captured step ------------------------------------------------------------------------------------------------
def _batches():
    from future_od.datasets.synthetic import make_batch
    return (make_batch(2, 3, 96, 128, seed=11, max_boxes=9, device=DEV),
            make_batch(2, 3, 96, 128, seed=12, max_boxes=20, device=DEV))       # other targets, one signature


def _grads(model):
    torch.cuda.synchronize()
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.requires_grad}


def _params(model):
    torch.cuda.synchronize()
    return {n: p.detach().clone() for n, p in model.named_parameters()}


def _differing(a, b):
    assert set(a) == set(b)
    return [k for k in a if not torch.equal(a[k], b[k])]


def _graphed(dtype, accumulate, **kw):
    from future_od.graph import GraphedStep
    from test_graph_gpu import _build
    model, opt = _build(dtype)
    return model, opt, GraphedStep(model, opt, warmup=2, rollback_warmup=True, accumulate=accumulate, **kw)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_same_batch_twice_is_one_plain_step(dtype):
    """(g + g) * 0.5 == g bit for bit: two micro-batches of the same batch leave the gradient of one, and the update is
    the one an unaccumulated captured step makes."""
    ops.set_deterministic(True)
    d, _ = _batches()
    model, opt, step = _graphed(dtype, 2)
    start = _params(model)
    step(d)
    g1 = _grads(model)
    assert len(g1) == sum(1 for p in model.parameters() if p.requires_grad)
    assert step.pending == 1 and opt._step_no == 0 and not _differing(start, _params(model))
    step(d)
    assert step.pending == 0 and opt._step_no == 1
    bad = _differing(g1, _grads(model))
    assert not bad, (len(bad), bad[:8])
    (g,) = step._graphs.values()
    assert g["accum"] is not None and g["record"].of("grad accumulator") == [g["accum"]]
    plain_model, plain_opt, plain = _graphed(dtype, 1)
    plain(d)
    assert plain_opt._step_no == 1 and next(iter(plain._graphs.values())).get("accum") is None
    bad = _differing(_params(model), _params(plain_model))
    assert not bad and _differing(start, _params(model)), (len(bad), bad[:8])
    for (n, p), q in zip(model.named_parameters(), plain_model.parameters()):
        if p.requires_grad:
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(opt.state[p][k], plain_opt.state[q][k]), (k, n)


def test_three_micro_batches_leave_their_ordered_mean():
    ops.set_deterministic(True)
    d1, d2 = _batches()
    model, opt, step = _graphed("bf16", 3)
    step(d1)
    g1 = _grads(model)
    step(d2)
    g2 = _grads(model)
    assert _differing(g1, g2)                                    # other targets: another gradient
    step(d1)
    got = _grads(model)                                          # (AdamW does not write gradients)
    third = torch.tensor(1.0 / 3.0, dtype=torch.float32, device=DEV)
    want = {n: ((g1[n] + g2[n]) + g1[n]) * third for n in g1}
    bad = _differing(got, want)
    assert not bad, (len(bad), bad[:8])
    assert opt._step_no == 1 and step.pending == 0


def test_cycle_bookkeeping_with_an_ema_attached():
    from future_od.optim import WeightEMA
    ops.set_deterministic(True)
    d1, d2 = _batches()
    model, opt, step = _graphed("bf16", 3)
    ema = WeightEMA(model)
    opt.attach_ema(ema)
    base = getattr(opt, "_step_no", 0)
    prev = _params(model)
    for call in range(1, 8):
        if call == 5:                                            # mid-cycle: takes effect at the cycle's update
            for grp in opt.param_groups:
                grp["lr"] = 3e-5
        step(d1 if call % 2 else d2)
        now = _params(model)
        moved = bool(_differing(prev, now))
        assert moved == (call in (3, 6)), call
        assert step.pending == call % 3
        if call == 5:                                            # not yet: the captured plan still reads the old rate
            (g,) = step._graphs.values()
            assert torch.equal(g["plan"]["tab"][2][:, 0].cpu(), torch.full((len(g["plan"]["params"]),), 1e-4))
        prev = now
    assert opt._step_no == base + 2 and ema.num_updates == 2
    assert step.pending == 1 and len(step._graphs) == 1 and step.replays == 7
    (g,) = step._graphs.values()
    assert g["plan"] is not None
    assert torch.equal(g["plan"]["tab"][2][:, 0].cpu(), torch.full((len(g["plan"]["params"]),), 3e-5))
    step.reset_cycle()
    assert step.pending == 0


def test_another_signature_inside_a_cycle_is_refused_before_anything_runs():
    from future_od.datasets.synthetic import make_batch
    ops.set_deterministic(True)
    d, _ = _batches()
    other = make_batch(1, 3, 96, 128, seed=22, max_boxes=9, device=DEV)
    model, opt, step = _graphed("bf16", 2)
    step(d)
    before, grads = _params(model), _grads(model)
    with pytest.raises(RuntimeError, match="signature"):
        step(other)
    assert step.pending == 1 and opt._step_no == 0 and len(step._graphs) == 1 and step.replays == 1
    assert not _differing(before, _params(model)) and not _differing(grads, _grads(model))
    step(d)                                                      # the open cycle is still good
    assert step.pending == 0 and opt._step_no == 1


def test_every_micro_batch_draws_its_own_dropout_masks_and_the_run_repeats():
    ops.set_deterministic(True)
    d, _ = _batches()
    runs = []
    for _ in range(2):
        model, opt, step = _graphed("bf16", 2)
        model.train()
        Fn.manual_seed(0)
        step(d)
        g1 = _grads(model)
        step(d)
        g = _grads(model)
        weights = [n for n, t in g1.items() if t.dim() >= 2 and (".transformer.layers" in n or ".decoder.layers" in n)
                   and bool(t.any())]
        assert len(weights) > 40
        same = [n for n in weights if torch.equal(g[n], g1[n])]
        assert not same, same[:8]                                # new masks in the second micro-batch
        state = dict(("grad " + n, t) for n, t in g.items())
        state.update(("param " + n, t) for n, t in _params(model).items())
        runs.append(state)
    bad = _differing(runs[0], runs[1])
    assert not bad, (len(bad), bad[:8])
    ops.DROP_BASE = None


# ---- two ranks --------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, q):
    """Two cycles of accumulate=2 on the data-parallel captured step, ranks built as test_parallel_gpu._graph_worker
    builds them (gloo, both on cuda:0, different shards per rank), with every `_all_reduce` call counted per step call."""
    import faulthandler
    faulthandler.dump_traceback_later(150, exit=True)          # a hung collective says where and ends the test
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "future-object-detection_amd"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from future_od.datasets.synthetic import make_batch
        from future_od.graph import GraphedStep
        from future_od.models.st_detr import SpatioTemporalDETRArgs
        from future_od.optim import FusedAdamW
        from runs._model import build_model
        dev = torch.device("cuda", 0)
        detr = SpatioTemporalDETRArgs(num_classes=8, num_queries=16, lr_backbone=1e-4, pretrained_backbone=False,
                                      backbone="resnet18", enc_layers=1, dec_layers=2)
        torch.manual_seed(11)
        args = SimpleNamespace(device=dev, distributed=False, compute_dtype="fp32", num_images=2, backbone="resnet18")
        model = build_model(args, detr)
        model.eval()
        opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=1e-4, max_norm=0.1)
        batches = [make_batch(1, 3, 64, 96, seed=300 + 10 * i + rank, device=dev, max_boxes=5) for i in range(4)]
        step = GraphedStep(model, opt, warmup=2, data_parallel=True, rollback_warmup=True, accumulate=2)
        step.broadcast_parameters()
        start = [p.detach().clone() for p in model.parameters()]
        seen, inner = [], step._all_reduce

        def counted(t, *a, **kw):
            seen.append(t.numel())
            return inner(t, *a, **kw)
        step._all_reduce = counted
        calls = []
        for b in batches:
            del seen[:]
            step(b)
            calls.append(list(seen))
        torch.cuda.synchronize()
        (g,) = step._graphs.values()
        spread = 0.0
        for p in model.parameters():
            lo, hi = p.detach().clone(), p.detach().clone()
            dist.all_reduce(lo, op=dist.ReduceOp.MIN)
            dist.all_reduce(hi, op=dist.ReduceOp.MAX)
            spread = max(spread, float((hi - lo).abs().max()))
        changed = sum(1 for p, s in zip(model.parameters(), start) if not torch.equal(p, s))
        q.put((rank, spread, calls, [t.numel() for t in g["targets"]], step.overlap, opt._step_no, step.pending, changed))
    except BaseException:                                       # the other rank must not wait for a collective forever
        import traceback
        q.put((rank, "error", traceback.format_exc()))
        os._exit(1)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_reduce_the_gradients_once_per_cycle():
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    for _ in range(world):
        r = q.get(timeout=260)
        if r[1] == "error":
            for p in procs:
                p.kill()
            raise AssertionError(f"rank {r[0]} failed:\n{r[2]}")
        res.append(r)
    res.sort()
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, spread, calls, targets, overlap, steps, pending, changed in res:
        assert spread == 0.0, (rank, spread)                   # every rank applied the same averaged gradients
        assert overlap is False and steps == 2 and pending == 0 and changed > 50
        assert targets and max(targets) > 1 << 20 and 1 not in targets
        # call 1 = the eager warm-up steps (each reduces num_boxes and the gradients), the capture's and the replay's
        # num_boxes; no gradient is reduced for the replayed micro-batch 1
        assert calls[0][-2:] == [1, 1] and calls[0][-3] != 1, (rank, calls[0][-8:])
        assert calls[1] == [1] + targets, (rank, calls[1])     # micro-batch 2: num_boxes, then the cycle's one reduce
        assert calls[2] == [1], (rank, calls[2])               # micro-batch 1 of cycle 2: num_boxes only
        assert calls[3] == [1] + targets, (rank, calls[3])
    assert res[0][2][1:] == res[1][2][1:] and res[0][3] == res[1][3]


# ---- the Trainer ------------------------------------------------------------------------------------------------------
class _Loader(list):
    batch_size = 2


@pytest.mark.parametrize("graphed", [True, False])
def test_trainer_updates_once_per_cycle_and_drops_an_open_one(graphed, tmp_path, capsys):
    from future_od import switches
    from future_od.datasets.synthetic import make_batch
    from future_od.models.st_detr import SpatioTemporalDETRArgs
    from future_od.trainer import Trainer
    from runs._helper import get_lr_func, setup_optimizer
    from runs._model import build_model
    args = SimpleNamespace(device=DEV, distributed=False, compute_dtype="bf16", backbone="resnet18")
    detr = SpatioTemporalDETRArgs(num_classes=8, num_queries=32, lr_backbone=1e-4, enc_layers=1, dec_layers=2,
                                  pretrained_backbone=False)
    batches = [make_batch(2, 3, 96, 128, seed=50 + i, max_boxes=5, device=DEV) for i in range(5)]
    with switches.override(FOD_GRAPH_TRAIN=int(graphed)):
        for items, dropped in ((4, 0), (5, 1)):
            torch.manual_seed(0)
            model = build_model(args, detr)
            sched, opt = setup_optimizer(detr, model, get_lr_func(4))
            tr = Trainer(model, opt, sched, _Loader(batches[:items]), {"val": _Loader(batches[:1])}, str(tmp_path),
                         str(tmp_path), "t", DEV, print_interval=2, visualization_epochs=[], visualization_iterations=[],
                         category_dict={}, checkpoint_epochs=False, is_master=True, max_norm=detr.max_norm)
            tr.set_accumulate(2)
            start = [p.detach().clone() for p in model.parameters()]
            tr.train(1)
            out = capsys.readouterr().out
            assert opt._step_no == 2 and tr._training_iterations == items, (items, opt._step_no)
            assert (getattr(tr, "_graphed", None) not in (None, False)) == graphed, out[-2000:]
            assert ("gradient accumulation: dropped 1 micro-batch" in out) == bool(dropped), out[-2000:]
            assert (tr._graphed.pending if graphed else tr._eager_pending) == 0
            assert any(not torch.equal(p, s) for p, s in zip(model.parameters(), start))
            hist = tr._stats["train labels loss"].history
            assert len(hist) == 1 and hist[0] == hist[0]
