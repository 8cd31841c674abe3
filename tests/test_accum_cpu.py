"""Gradient accumulation, the parts that need no GPU: the entry point's prototype as the binding reads it from
include/fod_ext.h, the ABI version, the argument checks that come before any launch, and the `accumulate` settings of
GraphedStep, the Trainer and the 500 ms run script."""
import os
import re

import pytest
import torch

from future_od.native import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, F = "pointer", "int", "float"


def test_prototype_is_read_from_the_second_header():
    assert abi.EXT_PROTOTYPES["fod_multi_accum"] == (I, [P, P, P, P, I, I, F, P])
    assert "fod_multi_accum" not in abi.PROTOTYPES and "fod_multi_accum" not in open(abi.HEADER_PATH).read()
    from future_od.native import lib as L
    assert "fod_multi_accum" in L.EXT_SIGNATURES and "fod_multi_accum" in L._ENTRY
    fn = L.LIB.fod_multi_accum
    assert fn.restype is abi.CTYPE[I] and list(fn.argtypes) == [abi.CTYPE[k] for k in (P, P, P, P, I, I, F, P)]


def test_abi_version_moved_with_the_entry_point():
    from future_od.native import lib as L
    hdr = open(os.path.join(ROOT, "include", "fod.h")).read()
    assert int(re.search(r"#define FOD_ABI_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == L.LIB.fod_abi_version() >= 11


@pytest.mark.parametrize("args,word", [
    ((None, 1, 1, 1, 1, 0, 1.0), "bad args"),              # a null table (each in turn below)
    ((1, None, 1, 1, 1, 0, 1.0), "bad args"),
    ((1, 1, None, 1, 1, 1, 1.0), "bad args"),
    ((1, 1, 1, None, 1, 2, 0.5), "bad args"),
    ((1, 1, 1, 1, 0, 0, 1.0), "bad args"),                 # no blocks
    ((1, 1, 1, 1, 1, 3, 1.0), "mode"),
    ((1, 1, 1, 1, 1, -1, 1.0), "mode"),
    ((1, 1, 1, 1, 1, 2, 0.0), "scale"),
    ((1, 1, 1, 1, 1, 2, -0.5), "scale"),
    ((1, 1, 1, 1, 1, 2, float("inf")), "scale"),
    ((1, 1, 1, 1, 1, 0, float("nan")), "scale"),
])
def test_arguments_are_refused_before_any_launch(args, word):
    """The non-null 'tables' are the address 1: a launch would fault, so a clean non-zero return is the check itself
    (and this machine has no device to launch on)."""
    from future_od.native import lib as L
    rc = L.LIB.fod_multi_accum(*args, None)
    assert rc != 0
    text = L.last_error()
    assert "multi_accum" in text and word in text, text
    with pytest.raises(L.FodError, match="multi_accum"):
        L.call("fod_multi_accum", *args, None)


class _Model:
    training = False


@pytest.mark.parametrize("bad", [0, -2, 1.5, 2.0, "2", None, True])
def test_graphed_step_refuses_what_is_not_a_positive_integer(bad):
    from future_od.graph import GraphedStep
    with pytest.raises(ValueError, match="accumulate"):
        GraphedStep(_Model(), object(), accumulate=bad)


def test_graphed_step_cycle_state_starts_closed():
    from future_od.graph import GraphedStep
    for n in (1, 3):
        step = GraphedStep(_Model(), object(), accumulate=n)
        assert step.accumulate == n and step.pending == 0
        step.pending = 2
        step.reset_cycle()
        assert step.pending == 0
    assert GraphedStep(_Model(), object()).accumulate == 1          # the default: today's step
    # accumulating: the backward pass is not split for an overlapped all-reduce, whatever the switch says
    assert GraphedStep(_Model(), object(), accumulate=2).overlap is False


def test_accumulator_refuses_host_tensors_and_a_one_batch_cycle():
    from future_od.native.lib import FodError
    from future_od.optim import GradAccumulator
    with pytest.raises(FodError, match="float32 tensors on one device"):
        GradAccumulator([torch.zeros(4)])                           # no fallback that adds on the host
    with pytest.raises(FodError, match="no tensors"):
        GradAccumulator([])
    acc = GradAccumulator.__new__(GradAccumulator)
    for n in (1, 0, 2.5):
        with pytest.raises(ValueError):
            acc.finish(n)


def test_run_script_takes_accumulate():
    import importlib
    run = importlib.import_module("runs.nusc_spatiotemporal_imu_500ms")
    assert run.build_parser().parse_args(["--accumulate", "4"]).accumulate == 4
    assert run.build_parser().parse_args([]).accumulate == 1


class _FakeModel:
    def get_stat_idfs(self):
        return []


def test_trainer_setting():
    from future_od.trainer import Trainer
    args = (_FakeModel(), object(), None, [0], {"val": [0]}, "", "", "t", "cpu", 1, [], [], {})
    tr = Trainer(*args)
    assert tr._accumulate == 1
    assert tr.set_accumulate(4) is tr and tr._accumulate == 4
    for bad in (0, 1.5, "2", True):
        with pytest.raises(ValueError):
            tr.set_accumulate(bad)
    assert tr._accumulate == 4
