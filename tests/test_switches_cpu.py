"""The Python-side switch table (future_od/switches.py): every FOD_* name future_od reads is a row of it and is read
nowhere else; defaults and the parsing rule of each kind, in fresh processes; set / override; the rows consumed while
future_od.native is imported; and no name shared with the library's table (csrc/knobs.h)."""
import ctypes
import glob
import json
import os
import re
import subprocess
import sys

import pytest

from future_od import switches
from future_od.switches import SW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "future-object-detection_amd")

ON_NAMES = ["FOD_LINEAR_KEEP", "FOD_FUSED_MLP2", "FOD_RES_GRAD_QUEUE", "FOD_FUSED_LINEAR_NORM", "FOD_FUSED_LINEAR_THEN",
            "FOD_FUSED_LINEAR_PRE", "FOD_GROUP_RESIDUAL", "FOD_IMU_BATCHED", "FOD_DKV_QUEUE", "FOD_FUSED_STEM_POOL",
            "FOD_WGRAD_QUEUE", "FOD_WGRAD_QUEUE_LONG", "FOD_GRAPH_TRAIN", "FOD_GRAPH_EVAL", "FOD_DEVICE_MATCH", "FOD_FASTCALL"]
OFF_NAMES = ["FOD_DETERMINISTIC", "FOD_GRAD_BF16", "FOD_GRAPH_TIMING", "FOD_WGRAD_QUEUE_EAGER", "FOD_IMU_COLLAPSED_TRAIN",
             "FOD_DDP_TORCH_INIT"]
DEFAULTS = dict({n: True for n in ON_NAMES}, **{n: False for n in OFF_NAMES},
                FOD_FUSED_LINEAR_NORM_ROWS=1024, FOD_WGRAD_LONG_ROWS=2048, FOD_FRONT_FRAMES=0,
                FOD_ATTN_FP8="off", FOD_FUSED_BOTTLENECK="2", FOD_GRAPH_OVERLAP_MODE="async", FOD_ASYNC_MATCH="1",
                FOD_GRAPH_OVERLAP=None)
CONSTRUCT = {"FOD_GRAPH_OVERLAP", "FOD_GRAPH_OVERLAP_MODE", "FOD_GRAD_BF16", "FOD_DDP_TORCH_INIT", "FOD_WGRAD_QUEUE",
             "FOD_WGRAD_QUEUE_EAGER", "FOD_WGRAD_QUEUE_LONG", "FOD_WGRAD_LONG_ROWS", "FOD_FASTCALL"}
AT_IMPORT = ["FOD_FASTCALL", "FOD_WGRAD_QUEUE", "FOD_WGRAD_QUEUE_EAGER", "FOD_WGRAD_QUEUE_LONG", "FOD_WGRAD_LONG_ROWS"]


def _fresh(**env_values):
    """The table's values in a fresh process whose environment holds exactly these FOD_* variables."""
    code = ("import json, sys; sys.path.insert(0, sys.argv[1])\n"
            "from future_od.switches import SW\nprint(json.dumps(vars(SW)))\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("FOD_")}
    env.update(env_values)
    r = subprocess.run([sys.executable, "-c", code, PKG], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_source_reads_the_environment_only_in_the_table():
    from future_od.native import abi
    from future_od.native import lib as L
    known = set(switches.TABLE) | set(abi.CONSTANTS)
    files = glob.glob(os.path.join(PKG, "future_od", "**", "*.py"), recursive=True)
    assert len(files) > 30
    for path in files:
        src = open(path).read()
        if os.path.basename(path) != "switches.py":
            for line in src.splitlines():
                assert not (("os.environ" in line or "getenv" in line) and "FOD_" in line), (path, line)
        for token in sorted(set(re.findall(r"FOD_[A-Z0-9_]+", src))):
            if token.endswith("_"):                   # prose about a family of header constants ("FOD_ROUTE_*")
                assert any(name.startswith(token) for name in abi.CONSTANTS), (path, token)
            elif token not in known:
                L.knob(token)                         # raises for a name that is not the library's either


def test_table_rows():
    assert len(switches.ROWS) == len(switches.TABLE) == len(DEFAULTS) == 30
    for row in switches.ROWS:
        assert row.default == DEFAULTS[row.name] and row.doc, row.name
        assert row.when == ("construct" if row.name in CONSTRUCT else "use"), row.name
    assert {r.name for r in switches.ROWS if r.kind == switches.ON} == set(ON_NAMES)
    assert {r.name for r in switches.ROWS if r.kind == switches.OFF} == set(OFF_NAMES)


def test_defaults_in_a_clean_environment():
    assert _fresh() == DEFAULTS


def test_parsing_on_unless_zero():
    for text, want in (("", True), ("false", True), ("2", True), ("1", True), ("0", False)):
        got = _fresh(**{n: text for n in ON_NAMES})
        assert all(got[n] is want for n in ON_NAMES), (text, got)


def test_parsing_off_unless_one():
    for text, want in (("true", False), ("2", False), ("0", False), ("", False), ("1", True)):
        got = _fresh(**{n: text for n in OFF_NAMES})
        assert all(got[n] is want for n in OFF_NAMES), (text, got)


def test_parsing_integers_text_and_three_state():
    got = _fresh(FOD_FRONT_FRAMES="3", FOD_FUSED_LINEAR_NORM_ROWS="16", FOD_WGRAD_LONG_ROWS=" 512",
                 FOD_ATTN_FP8="long", FOD_FUSED_BOTTLENECK="0", FOD_GRAPH_OVERLAP_MODE="after", FOD_ASYNC_MATCH="2",
                 FOD_GRAPH_OVERLAP="1")
    assert (got["FOD_FRONT_FRAMES"], got["FOD_FUSED_LINEAR_NORM_ROWS"], got["FOD_WGRAD_LONG_ROWS"]) == (3, 16, 512)
    assert (got["FOD_ATTN_FP8"], got["FOD_FUSED_BOTTLENECK"], got["FOD_GRAPH_OVERLAP_MODE"], got["FOD_ASYNC_MATCH"]) \
        == ("long", "0", "after", "2")
    assert got["FOD_GRAPH_OVERLAP"] is True
    assert _fresh(FOD_FRONT_FRAMES="0")["FOD_FRONT_FRAMES"] == 0
    assert _fresh()["FOD_GRAPH_OVERLAP"] is None
    for text in ("0", "yes", ""):
        assert _fresh(FOD_GRAPH_OVERLAP=text)["FOD_GRAPH_OVERLAP"] is False, text


@pytest.mark.parametrize("name", ["FOD_FUSED_LINEAR_NORM_ROWS", "FOD_WGRAD_LONG_ROWS", "FOD_FRONT_FRAMES"])
def test_a_malformed_integer_raises_and_names_the_variable(name):
    code = "import sys; sys.path.insert(0, sys.argv[1]); import future_od.switches"
    r = subprocess.run([sys.executable, "-c", code, PKG], env=dict(os.environ, **{name: "12x"}), capture_output=True,
                       text=True, timeout=60)
    assert r.returncode != 0 and "ValueError" in r.stderr and name in r.stderr, r.stderr[-2000:]
    with pytest.raises(ValueError, match="FOD_FRONT_FRAMES"):
        switches.set("FOD_FRONT_FRAMES", "many")


def test_override_restores_nests_and_parses():
    before = dict(vars(SW))
    with switches.override(FOD_FUSED_MLP2=0, FOD_ATTN_FP8="all", FOD_FRONT_FRAMES="2", FOD_GRAPH_OVERLAP="yes"):
        assert (SW.FOD_FUSED_MLP2, SW.FOD_ATTN_FP8, SW.FOD_FRONT_FRAMES, SW.FOD_GRAPH_OVERLAP) == (False, "all", 2, False)
        with switches.override(FOD_FUSED_MLP2="2", FOD_DETERMINISTIC=True, FOD_FUSED_BOTTLENECK=0):
            assert (SW.FOD_FUSED_MLP2, SW.FOD_DETERMINISTIC, SW.FOD_FUSED_BOTTLENECK) == (True, True, "0")
            with switches.override(FOD_FUSED_MLP2="0", FOD_DETERMINISTIC=2):        # "2" is not "1": off
                assert (SW.FOD_FUSED_MLP2, SW.FOD_DETERMINISTIC) == (False, False)
            assert (SW.FOD_FUSED_MLP2, SW.FOD_DETERMINISTIC) == (True, True)
        assert (SW.FOD_FUSED_MLP2, SW.FOD_DETERMINISTIC, SW.FOD_FUSED_BOTTLENECK) == (False, before["FOD_DETERMINISTIC"], before["FOD_FUSED_BOTTLENECK"])
    assert vars(SW) == before
    with pytest.raises(ZeroDivisionError):
        with switches.override(FOD_GROUP_RESIDUAL=False, FOD_ASYNC_MATCH=2):
            assert (SW.FOD_GROUP_RESIDUAL, SW.FOD_ASYNC_MATCH) == (False, "2")
            1 / 0
    assert vars(SW) == before
    for same in (0, "0", False):
        with switches.override(FOD_FUSED_MLP2=same):
            assert SW.FOD_FUSED_MLP2 is False


def test_unknown_names_raise_and_change_nothing():
    before = dict(vars(SW))
    with pytest.raises(LookupError):
        switches.set("FOD_NO_SUCH_SWITCH", 1)
    with pytest.raises(LookupError):
        with switches.override(FOD_FUSED_MLP2=0, FOD_NO_SUCH_SWITCH=1):
            raise AssertionError("entered")
    for knob in ("FOD_TN_BIG", "FOD_NT_SMALL"):                    # the library's: another table
        with pytest.raises(LookupError, match=r"lib\.knobs"):
            switches.set(knob, 0)
        with pytest.raises(LookupError, match=r"lib\.knobs"):
            with switches.override(**{knob: 0}):
                raise AssertionError("entered")
    assert vars(SW) == before and not hasattr(SW, "FOD_TN_BIG")


def test_set_none_returns_to_the_value_of_import():
    code = ("import sys; sys.path.insert(0, sys.argv[1])\n"
            "from future_od import switches\nfrom future_od.switches import SW\n"
            "switches.set('FOD_FUSED_MLP2', 1); switches.set('FOD_ATTN_FP8', 'all'); switches.set('FOD_FRONT_FRAMES', 5)\n"
            "a = (SW.FOD_FUSED_MLP2, SW.FOD_ATTN_FP8, SW.FOD_FRONT_FRAMES)\n"
            "for n in ('FOD_FUSED_MLP2', 'FOD_ATTN_FP8', 'FOD_FRONT_FRAMES'): switches.set(n, None)\n"
            "print(a, (SW.FOD_FUSED_MLP2, SW.FOD_ATTN_FP8, SW.FOD_FRONT_FRAMES))\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("FOD_")}
    env.update(FOD_FUSED_MLP2="0", FOD_ATTN_FP8="long")
    r = subprocess.run([sys.executable, "-c", code, PKG], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "(True, 'all', 5) (False, 'long', 0)", r.stdout + r.stderr[-2000:]


def test_rows_consumed_at_import_refuse_a_later_change():
    from future_od.native import wgrad                             # noqa: F401  (the consumers are imported)
    before = dict(vars(SW))
    for name in AT_IMPORT:
        hint = "before the process starts" if name == "FOD_FASTCALL" else "WGRADS"
        with pytest.raises(RuntimeError, match=hint):
            switches.set(name, 0)
        with pytest.raises(RuntimeError, match=hint):
            with switches.override(**{name: 0}):
                raise AssertionError("entered")
    assert vars(SW) == before


def test_the_two_tables_share_no_name():
    from future_od.native import lib as L
    buf = ctypes.create_string_buffer(32)
    for name in switches.TABLE:
        assert L.LIB.fod_knob_get(name.encode(), buf, 32) != 0, name
