"""Lifetime of what a captured graph bakes in (future_od/native/capture.py), without a device: a capture record keeps
the prepared operands, refresh tables and arena buffers that were used while it was open; what no record holds is freed
as soon as its producer replaces or drops it."""
import gc
import weakref

import pytest
import torch


@pytest.fixture
def native(monkeypatch):
    """The native layer with its launches stubbed out and a prepared-operand store of the test's own."""
    from future_od.native import capture
    from future_od.native import ops
    from future_od.native import prepared
    monkeypatch.setattr(prepared.L, "call", lambda *a, **k: None)
    monkeypatch.setattr(ops, "stream", lambda: 0)
    monkeypatch.setattr(prepared, "PREP", prepared._Prepared())
    assert capture._open is None
    return capture, prepared


def _weight(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Parameter(torch.randn(24, 16))


def _prepare(prep, w):
    """Request the operand of `w`: builds its entry and launches (stub) a refresh from a table of its own.
    -> weak references to the entry's value tensor and to the table's device job array."""
    value = prep.prep_linear(w, torch.float32, False)
    table = list(prep.PREP._tables.values())[-1]
    assert table[4][0][1] is value                    # the table built last is the one that fills this entry
    return weakref.ref(value), weakref.ref(table[0])


def test_a_record_keeps_what_was_used_while_it_was_open(native):
    capture, prep = native
    w = _weight()
    with capture.Record() as record:
        value, table = _prepare(prep, w)
    del w                 # (a live parameter's memo keeps its own entry, and the store it was made in, for the fast path)
    assert record.of("prepared operands") and record.of("refresh table")
    prep.PREP.clear()
    gc.collect()
    assert value() is not None and table() is not None
    del record
    gc.collect()
    assert value() is None and table() is None


def test_without_a_record_clear_frees(native):
    capture, prep = native
    w = _weight()
    value, table = _prepare(prep, w)
    del w
    prep.PREP.clear()
    gc.collect()
    assert value() is None and table() is None
    assert not capture.FOREIGN


def test_an_evicted_refresh_table_survives_only_in_a_record(native):
    capture, prep = native
    weights = [_weight(i) for i in range(24)]
    with capture.Record() as record:
        _, held = _prepare(prep, weights[0])
    _, loose = _prepare(prep, weights[1])
    for w in weights[2:]:                             # 22 further stale sets, one table each: the cap of 16 is passed
        _prepare(prep, w)
    assert len(prep.PREP._tables) < 16
    gc.collect()
    assert held() is not None and loose() is None
    assert record.of("refresh table")[0][0] is held()
    del record
    gc.collect()
    assert held() is None


def test_an_outgrown_arena_buffer_survives_only_in_a_record(native):
    capture, prep = native

    def outgrow(arena):
        old = weakref.ref(arena.buf)
        arena.high = 2 * arena.buf.numel()
        arena.recycle("cpu")
        assert arena.buf is not old() and arena.buf.numel() >= arena.cap // 2
        gc.collect()
        return old

    from future_od.native.arena import _ZeroArena
    arena = _ZeroArena()
    arena.recycle("cpu")
    assert outgrow(arena)() is None
    with capture.Record() as record:
        old = outgrow(arena)
    assert old() is not None and record.of("gradient arena")[0] is old()
    del record
    gc.collect()
    assert old() is None


def test_a_record_asks_the_providers_when_it_closes(native):
    capture, prep = native
    w = _weight()
    value, _ = _prepare(prep, w)                        # built BEFORE the record opens, as a capture's warm-up does
    with capture.Record() as record:
        assert prep.prep_linear(w, torch.float32, False) is value()        # the memo fast path: holds nothing itself
        assert not record.held
    assert [id(o) for o in record.of("prepared operands")] == [id(prep.PREP._store)]
    del w
    prep.PREP.clear()
    gc.collect()
    assert value() is not None


def test_hold_outside_a_record_keeps_nothing(native):
    capture, prep = native
    t = torch.zeros(4)
    ref = weakref.ref(t)
    assert capture.hold("anything", t) is None and capture.hold_or_ask("anything", t) is False
    assert capture._open is None and not capture.FOREIGN
    del t
    gc.collect()
    assert ref() is None
