"""Weight EMA, the parts that need no GPU: the update weight restated in python against hand values, the second header
(include/fod_ext.h) read by the project's reader and served by the binding beside -- never inside -- fod.h's tables, the
state-dict schema, and the Trainer's `ema=` keyword."""
import inspect
import os

import numpy as np
import pytest
import torch

from future_od.native import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, F = "pointer", "int", "float"
EXT_ENTRIES = ("fod_multi_ema", "fod_multi_swap")


def ema_weight(u, decay, warmup):
    """The weight of update number u as include/fod_ext.h states it: the decay the kernel is handed is a float32, the
    warm-up bound and the minimum are formed in double, and w = float32(1 - d)."""
    d = float(np.float32(decay))
    if warmup:
        d = min(d, (1.0 + u) / (10.0 + u))
    return np.float32(1.0 - d)


def test_update_weight_hand_values():
    assert ema_weight(1, 0.9998, True) == np.float32(1.0 - 2.0 / 11.0) == np.float32(9.0 / 11.0)
    assert ema_weight(10, 0.9998, True) == np.float32(1.0 - 11.0 / 20.0) == np.float32(0.45)
    d32 = float(np.float32(0.9998))                       # 0.99980002641677856...: what a float argument carries
    plain = np.float32(1.0 - d32)
    assert abs(float(plain) - 1.9997358e-4) < 1e-11
    # (1 + u) / (10 + u) reaches the decay at u = (10 d - 1) / (1 - d): 44990 for 0.9998 itself, a little later for
    # the float32 next to it
    cross = (10.0 * d32 - 1.0) / (1.0 - d32)
    assert 44990 < cross < 45000
    below, above = int(cross) - 1, int(cross) + 2
    assert ema_weight(below, 0.9998, True) == np.float32(1.0 - (1.0 + below) / (10.0 + below)) > plain
    assert ema_weight(above, 0.9998, True) == plain == ema_weight(100000, 0.9998, True)
    ws = [ema_weight(u, 0.9998, True) for u in (1, 2, 10, 1000, below, above, 100000)]
    assert all(a >= b for a, b in zip(ws, ws[1:]))
    for u in (1, 2, 10, 100000):                           # warm-up off: the decay from the first update on
        assert ema_weight(u, 0.9998, False) == plain
    assert ema_weight(5, 1.0, False) == 0.0 and ema_weight(5, 0.0, False) == 1.0 and ema_weight(5, 0.0, True) == 1.0


def test_the_second_header_reads_with_the_projects_reader():
    assert os.path.samefile(abi.EXT_HEADER_PATH, os.path.join(ROOT, "include", "fod_ext.h"))
    text = open(abi.EXT_HEADER_PATH).read()
    assert text.lstrip().startswith("/*") and "Why a second header" in text.split("*/")[0]
    known = abi.pointer_typedefs(open(abi.HEADER_PATH).read())
    assert "fod_stream_t" in known
    protos, structs, consts = abi.parse(text, known)
    assert protos == abi.EXT_PROTOTYPES and structs == {} and consts == {}
    for name in EXT_ENTRIES:
        assert name in protos, name
    assert protos["fod_multi_ema"] == (I, [P, P, P, P, I, P, F, I, P])
    assert protos["fod_multi_swap"] == (I, [P, P, P, P, I, P])
    with pytest.raises(abi.FodError, match="fod_stream_t"):          # it does not declare the stream type itself
        abi.parse(text)
    # fod.h's tables describe fod.h alone
    assert not set(protos) & set(abi.PROTOTYPES)
    assert abi._read()[0] == abi.PROTOTYPES and not set(protos) & set(abi.served(abi.PROTOTYPES))
    hdr = open(abi.HEADER_PATH).read()
    for name in protos:
        assert name not in hdr, name


def test_the_binding_serves_the_second_header_beside_the_first():
    from future_od.native import lib as L
    assert L.EXT_EXPORTS == sorted(abi.EXT_PROTOTYPES) and set(L.EXT_SIGNATURES) == set(abi.served(abi.EXT_PROTOTYPES))
    for name, (ret, args) in abi.EXT_PROTOTYPES.items():
        fn = getattr(L.LIB, name)                                   # exported by the built library, typed by the binding
        assert fn.restype is abi.CTYPE[ret] and list(fn.argtypes) == [abi.CTYPE[k] for k in args], name
        assert L.EXT_SIGNATURES[name] == [abi.CTYPE[k] for k in args]
        assert name in L._ENTRY
        assert name not in L.EXPORTS and name not in L.SIGNATURES and name not in L.FAST, name
    assert L.LIB.fod_abi_version() == abi.CONSTANTS["FOD_ABI_VERSION"] >= 10
    # call() serves them: null operands are rejected on the host, with the entry point's own text
    with pytest.raises(L.FodError, match="multi_ema"):
        L.call("fod_multi_ema", None, None, None, None, 0, None, 0.5, 1, None)
    with pytest.raises(L.FodError, match="multi_swap"):
        L.call("fod_multi_swap", None, None, None, None, 0, None)
    assert L.LIB.fod_multi_ema(1, 1, 1, 1, 1, 1, 1.5, 0, None) != 0 and "decay" in L.last_error()     # before any launch


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(3, 2)
        self.frozen = torch.nn.Linear(2, 2)
        self.frozen.weight.requires_grad_(False)
        self.register_buffer("stat", torch.ones(2))


def _host_ema(model, updates=0):
    """A WeightEMA over host tensors, put together by hand (the constructor refuses them: the update is a device
    kernel): everything but update() / applied() is plain tensor code."""
    from future_od.optim import WeightEMA
    ema = WeightEMA.__new__(WeightEMA)
    ema.decay, ema.warmup, ema._model, ema._applied = 0.99, True, model, False
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    ema._names, ema._params = [n for n, _ in named], [p for _, p in named]
    ema._ema = [p.detach().clone() for p in ema._params]
    ema._updates = torch.tensor([updates], dtype=torch.int64)
    return ema


def test_state_dict_schema_and_in_place_loading():
    from future_od.native.lib import FodError
    from future_od.optim import WeightEMA
    model = _Tiny()
    with pytest.raises(FodError, match="float32 parameters on one device"):
        WeightEMA(model)                                            # host parameters: refused, no fallback
    with pytest.raises(ValueError):
        WeightEMA(model, decay=1.5)
    ema = _host_ema(model, updates=7)
    names = ["a.weight", "a.bias", "frozen.bias"]                   # requires_grad parameters only, no buffer
    assert [n for n, _ in ema.named_tensors()] == names
    sd = ema.state_dict()
    assert set(sd) == {"decay", "warmup", "num_updates", "params"}
    assert (sd["decay"], sd["warmup"], sd["num_updates"]) == (0.99, True, 7) and list(sd["params"]) == names
    assert all(torch.equal(sd["params"][n], p) for n, p in model.named_parameters() if n in names)
    # loading copies in place: same tensors, same addresses
    other = _host_ema(_Tiny())
    before = [e.data_ptr() for e in other._ema]
    other.load_state_dict(sd)
    assert [e.data_ptr() for e in other._ema] == before and other.num_updates == 7
    assert all(torch.equal(e, sd["params"][n]) for n, e in other.named_tensors())
    for bad in ({k: v for k, v in sd["params"].items() if k != "a.bias"}, dict(sd["params"], extra=torch.zeros(1)),
                dict(sd["params"], **{"a.bias": torch.zeros(3)})):
        with pytest.raises(FodError):
            other.load_state_dict(dict(sd, params=bad))
    # the model's full state dict with the averaged values substituted: loads straight into a fresh model
    with torch.no_grad():
        ema._ema[0].add_(1.0)
    msd = ema.model_state_dict()
    assert list(msd) == list(model.state_dict())
    fresh = _Tiny()
    fresh.load_state_dict(msd)
    assert torch.equal(fresh.a.weight, model.a.weight + 1.0) and torch.equal(fresh.frozen.weight, model.frozen.weight)
    ema.reset()
    assert ema.num_updates == 0 and torch.equal(ema._ema[0], model.a.weight)
    # inside applied() the EMA's tensors hold the raw weights: its state is refused
    ema._applied = True
    for call in (ema.state_dict, ema.model_state_dict, ema.reset, lambda: ema.load_state_dict(sd), ema.update):
        with pytest.raises(RuntimeError, match="applied"):
            call()


class _FakeModel:
    def get_stat_idfs(self):
        return []


class _FakeOptimizer:
    max_norm = 0.0

    def attach_ema(self, ema):
        self.attached = ema


def test_trainer_takes_an_ema_and_is_unchanged_without():
    from future_od.optim import FusedAdamW
    from future_od.trainer import Trainer
    params = list(inspect.signature(Trainer.__init__).parameters.values())
    assert [p.name for p in params] == [
        "self", "model", "optimizer", "lr_sched", "train_loader", "val_loaders", "checkpoint_path", "visualization_path",
        "save_name", "device", "print_interval", "visualization_epochs", "visualization_iterations", "category_dict",
        "checkpoint_epochs", "gradient_clip_value", "distributed", "is_master", "wandb_config", "max_norm", "ema"]
    assert params[-1].default is None
    args = (_FakeModel(), None, None, [0], {"val": [0]}, "", "", "t", "cpu", 1, [], [], {})
    plain = object()                                     # an optimizer that knows nothing of EMAs: never asked
    assert Trainer(args[0], plain, *args[2:])._ema is None
    opt, ema = _FakeOptimizer(), object()
    tr = Trainer(args[0], opt, *args[2:], ema=ema)
    assert tr._ema is ema and opt.attached is ema
    # the optimizer: nothing attached by default; a step while the average is applied is refused before anything runs
    w = torch.nn.Parameter(torch.zeros(3))
    fused = FusedAdamW([w])
    assert fused._ema is None
    applied = _host_ema(_Tiny())
    applied._applied = True
    fused.attach_ema(applied)
    step_no = getattr(fused, "_step_no", 0)
    with pytest.raises(RuntimeError, match="applied"):
        fused.step()
    assert getattr(fused, "_step_no", 0) == step_no
    fused.attach_ema(None)
    assert fused._ema is None
