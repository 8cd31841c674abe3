"""The Python-side switches: ONE table, read from the environment once.

Every FOD_* variable that future_od itself looks at has a row here (the library's own knobs are the table of
csrc/knobs.h, behind lib.knob / lib.set_knob / lib.knobs; the two tables share no name).  The environment is read when
this module is first imported; afterwards only set() / override() change a value.  The values live in SW and are read
at the point of use: `SW.FOD_FUSED_MLP2` is one attribute lookup.  What a value was measured to do is written where it
is used.  Standard library only: native/lib.py needs FOD_FASTCALL before it loads anything.
"""
import contextlib
import os
import types
from collections import namedtuple


def _int(name, text):
    try:
        return int(text)
    except ValueError:
        raise ValueError(f"{name}={text!r} is not an integer") from None


# kinds: how a row's text becomes its value.  The rules differ on purpose: they are the expressions the reading sites
# have always used.  A variable that is not set gives the row's default.
ON = lambda name, text: text != "0"             # on unless "0": "", "false", "2" are all on
OFF = lambda name, text: text == "1"            # off unless "1": "true", "2" are off
INT = _int
TEXT = lambda name, text: text                  # as written; compared as text where it is used
TRISTATE = lambda name, text: text == "1"       # not set: None (a rule at the reading site decides); any other text: off
# when a row is consumed.  USE: looked up every time the decision is taken, override() works at any time.  CONSTRUCT:
# when an object is built (GraphedStep, FodDataParallel, the WGRADS singleton, the fast-call loader), which then
# carries the value as its own attribute
USE, CONSTRUCT = "use", "construct"
Row = namedtuple("Row", "name kind default when doc")

ROWS = (
    Row("FOD_LINEAR_KEEP", ON, True, USE, "0: a kept projection has two autograd consumers instead of linear_keep (experiments)"),
    Row("FOD_FUSED_MLP2", ON, True, USE, "0: the decoder's query_scale MLP and its product with the sine embedding as 2 GEMMs + a multiply"),
    Row("FOD_RES_GRAD_QUEUE", ON, True, USE, "0: every encoder layer sums the gradient of its per-frame IMU rows itself"),
    Row("FOD_FUSED_LINEAR_NORM", ON, True, USE, "0: output projection and post-norm of the decoder's attention blocks as two launches"),
    Row("FOD_FUSED_LINEAR_THEN", ON, True, USE, "0: the next cross-attention block's query-content projection as its own GEMM"),
    Row("FOD_FUSED_LINEAR_PRE", ON, True, USE, "0: that projection's input gradient by a GEMM of LinearKeepFn, not inside the fused backward"),
    Row("FOD_FUSED_LINEAR_NORM_ROWS", INT, 1024, USE, "rows up to which the fused projection + norm launches are used"),
    Row("FOD_ATTN_FP8", TEXT, "off", USE, "long: long-query bf16 attention runs the MX-fp8 forward; all: every bf16 attention without dropout"),
    Row("FOD_GROUP_RESIDUAL", ON, True, USE, "0: the self-attention's position adds as their own element-wise launches"),
    Row("FOD_IMU_BATCHED", ON, True, USE, "0: every encoder layer computes its IMU-token block itself"),
    Row("FOD_DKV_QUEUE", ON, True, USE, "0: every cross-attention block launches its own dk / dv pass"),
    Row("FOD_FUSED_STEM_POOL", ON, True, USE, "0: the frozen stem and its max-pool as two launches"),
    Row("FOD_FRONT_FRAMES", INT, 0, USE, "n > 0: frames per pass of the frozen front; 0: all frames at once"),
    Row("FOD_FUSED_BOTTLENECK", TEXT, "2", USE, "1: only a stage's first frozen bottleneck as one launch; 0: none"),
    Row("FOD_DETERMINISTIC", OFF, False, USE, "1: gradients summed in index order, bit-identical from run to run (ops.set_deterministic)"),
    Row("FOD_WGRAD_QUEUE", ON, True, CONSTRUCT, "0: every short weight gradient is its own launch; later: change WGRADS.enabled"),
    Row("FOD_WGRAD_QUEUE_EAGER", OFF, False, CONSTRUCT, "1: weight gradients queue in eagerly launched steps too; later: change WGRADS.eager"),
    Row("FOD_WGRAD_QUEUE_LONG", ON, True, CONSTRUCT, "0: the long Linear weight gradients do not share a launch; later: change WGRADS.long_enabled"),
    Row("FOD_WGRAD_LONG_ROWS", INT, 2048, CONSTRUCT, "rows per M-split of the long weight gradients' shared launch; later: change WGRADS.long_rows"),
    Row("FOD_FASTCALL", ON, True, CONSTRUCT, "0: every library call goes through ctypes, not the generated wrappers; set it before the process starts"),
    Row("FOD_IMU_COLLAPSED_TRAIN", OFF, False, USE, "1: the collapsed one-key IMU attention in train mode too (per-frame dropout masks)"),
    Row("FOD_DEVICE_MATCH", ON, True, USE, "0: the host assignment solver, asynchronous or blocking"),
    Row("FOD_ASYNC_MATCH", TEXT, "1", USE, "0: the host solver blocks the step; 2: it always parks, even when the costs have arrived (tests)"),
    Row("FOD_GRAPH_TRAIN", ON, True, USE, "0: the training loop launches every step eagerly"),
    Row("FOD_GRAPH_EVAL", ON, True, USE, "0: the evaluation loop launches every step eagerly"),
    Row("FOD_GRAPH_TIMING", OFF, False, USE, "1: a replayed step synchronises and prints the time of each of its phases"),
    Row("FOD_GRAPH_OVERLAP", TRISTATE, None, CONSTRUCT, "1 / other: gradient all-reduce beside the backward graph on / off; not set: GraphedStep's rule"),
    Row("FOD_GRAPH_OVERLAP_MODE", TEXT, "async", CONSTRUCT, "after: the overlapped all-reduce is launched after the backward graph (experiment)"),
    Row("FOD_GRAD_BF16", OFF, False, CONSTRUCT, "1: gradients are all-reduced as bf16"),
    Row("FOD_DDP_TORCH_INIT", OFF, False, CONSTRUCT, "1: FodDataParallel runs torch's DistributedDataParallel constructor"),
)
TABLE = {row.name: row for row in ROWS}
# consumed while future_od.native is imported: a later set() would silently do nothing, so it raises and says what to do
_AT_IMPORT = {"FOD_WGRAD_QUEUE", "FOD_WGRAD_QUEUE_EAGER", "FOD_WGRAD_QUEUE_LONG", "FOD_WGRAD_LONG_ROWS", "FOD_FASTCALL"}


def _parse(row, text):
    return row.default if text is None else row.kind(row.name, text)


SW = types.SimpleNamespace(**{row.name: _parse(row, os.environ.get(row.name)) for row in ROWS})
_IMPORTED = dict(vars(SW))          # what the environment or the default gave: set(name, None) returns to it


def _row(name):
    if name not in TABLE:
        raise LookupError(f"{name} is not a Python-side switch (future_od/switches.py); a knob of the library "
                          "(csrc/knobs.h) is changed with lib.set_knob / lib.knobs")
    if name in _AT_IMPORT:
        raise RuntimeError(f"{name} was consumed when future_od.native was imported -- {TABLE[name].doc}")
    return TABLE[name]


def set(name, value):
    """value: a Python value (False, 2) or the environment's text, parsed by the row's rule either way; None: back to
    what the environment or the default gave at import."""
    row = _row(name)
    text = str(int(value)) if isinstance(value, bool) else str(value)
    setattr(SW, name, _IMPORTED[name] if value is None else _parse(row, text))


@contextlib.contextmanager
def override(**values):
    """with override(FOD_FUSED_MLP2=0, FOD_ATTN_FP8="all"): ...  -- the previous values come back on exit."""
    old = {name: getattr(SW, _row(name).name) for name in values}
    try:
        for name, value in values.items():
            set(name, value)
        yield
    finally:
        vars(SW).update(old)
