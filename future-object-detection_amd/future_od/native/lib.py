"""ctypes binding of libfod_hip.so (include/fod.h, and the later entry points of include/fod_ext.h).

The HIP library IS the compute path: if it is missing or its ABI disagrees, importing this
module raises -- there is no CPU or eager-PyTorch fallback behind these calls.
"""
import contextlib
import ctypes as C
import os

from . import abi
from .abi import FodError
from ..switches import SW

LIB_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "lib", "libfod_hip.so"))

# every enumerator and integer macro of the header under its name without FOD_ (and without ROUTE_): F32, BF16, EW_*,
# NT_* / TN_* (FOD_ROUTE_*), CONV_*, ATTN_*, WS_* (fod_workspace_bytes kinds), ABI_VERSION, TN_DET_MAX_SPLITS, ...
globals().update({name[4:].replace("ROUTE_", "", 1): value for name, value in abi.CONSTANTS.items()})

_i, _l, _f, _p = C.c_int, C.c_long, C.c_float, C.c_void_p


def _struct(name, c_name):
    """ctypes mirror of `typedef struct c_name`: the header's fields in the header's order (pointers as addresses)."""
    return type(name, (C.Structure,), {"_fields_": [(field, abi.CTYPE[kind]) for field, kind in abi.STRUCTS[c_name]]})


Epilogue = _struct("Epilogue", "fod_epilogue")
ConvGeom = _struct("ConvGeom", "fod_conv_geom")
AttnShape = _struct("AttnShape", "fod_attn_shape")
PermuteJob = _struct("PermuteJob", "fod_permute_job")
TnJob = _struct("TnJob", "fod_tn_job")
NtRoute = _struct("NtRoute", "fod_nt_route")        # kernel is one of NT_SMALL / NT_128 / NT_BIG
TnRoute = _struct("TnRoute", "fod_tn_route")        # kernel is one of TN_SMALL / TN_128 / TN_BIG
AttnRoute = _struct("AttnRoute", "fod_attn_kernels")    # fwd / dq / dkv are one of ATTN_PLAIN / ATTN_LDS / ATTN_PREFETCH

EXPORTS = sorted(abi.PROTOTYPES)
# name -> argtypes of the entry points call() and the fast-call wrappers serve.  Struct arguments travel as addresses
# (C.addressof / None): plain ints are what the fast-call wrappers take.
SIGNATURES = {name: [abi.CTYPE[kind] for kind in args] for name, args in abi.served(abi.PROTOTYPES).items()}
# the same two tables for include/fod_ext.h; call() serves these through ctypes (there are no fast-call wrappers of them)
EXT_EXPORTS = sorted(abi.EXT_PROTOTYPES)
EXT_SIGNATURES = {name: [abi.CTYPE[kind] for kind in args] for name, args in abi.served(abi.EXT_PROTOTYPES).items()}


def _typed(lib, name):
    ret, args = abi.PROTOTYPES[name] if name in abi.PROTOTYPES else abi.EXT_PROTOTYPES[name]
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = abi.CTYPE[ret], [abi.CTYPE[kind] for kind in args]
    return fn


def _load():
    if not os.path.isfile(LIB_PATH):
        raise FodError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or future-object-detection_amd/build.sh). There is no fallback path.")
    # torch first: it ships its own libamdhip64.so, and the device memory and streams these entry points are handed come
    # from it.  Loaded the other way round (this module imported before torch, as __graft_entry__.build() does), the library
    # binds to the system runtime instead and its first launch fails with "no ROCm-capable device is detected"
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    built = _typed(lib, "fod_abi_version")()
    if built != abi.CONSTANTS["FOD_ABI_VERSION"]:
        raise FodError(f"libfod_hip.so ABI {built} != header ABI {abi.CONSTANTS['FOD_ABI_VERSION']}: rebuild")
    for name in EXPORTS + EXT_EXPORTS:
        if not hasattr(lib, name):
            raise FodError(f"libfod_hip.so does not export {name}: rebuild")
        _typed(lib, name)
    return lib


LIB = _load()


def last_error():
    buf = C.create_string_buffer(512)
    LIB.fod_last_error(buf, 512)
    return buf.value.decode("utf-8", "replace")


# ---- kernel-selection knobs (csrc/knobs.h): the library reads the FOD_* variables it looks at ONCE, at its first use;
# afterwards the environment does not reach it -- these do.  A captured graph keeps the kernels of its capture.
def knob(name):
    """The value in effect of a C-side knob, as text ("auto" where a rule decides)."""
    buf = C.create_string_buffer(32)
    if LIB.fod_knob_get(name.encode(), buf, 32) != 0:
        raise FodError(f"fod_knob_get failed: {last_error()}")
    return buf.value.decode()


def set_knob(name, value):
    """value None: back to the default."""
    if LIB.fod_knob_set(name.encode(), None if value is None else str(value).encode()) != 0:
        raise FodError(f"fod_knob_set failed: {last_error()}")


@contextlib.contextmanager
def knobs(**values):
    """with knobs(FOD_TN_BIG=2, FOD_TN_WS=0): ...  -- the previous values come back on exit."""
    old = {name: knob(name) for name in values}
    try:
        for name, value in values.items():
            set_knob(name, value)
        yield
    finally:
        for name, value in old.items():
            set_knob(name, value)


def _load_fast():
    """The generated CPython wrappers (csrc/fastcall.c, built next to the library): same entry points, ~5 us less
    host time per call than ctypes.  Optional: without them every call goes through ctypes (same library)."""
    import importlib.util
    path = os.path.join(os.path.dirname(LIB_PATH), "_fodfast.so")
    if not os.path.isfile(path) or not SW.FOD_FASTCALL:
        return {}
    spec = importlib.util.spec_from_file_location("_fodfast", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {name: getattr(mod, name) for name in SIGNATURES if hasattr(mod, name)}


FAST = _load_fast()
_ENTRY = {name: FAST.get(name, getattr(LIB, name)) for name in SIGNATURES}
_ENTRY.update({name: getattr(LIB, name) for name in EXT_SIGNATURES})


def _plain_call(name, *args):
    rc = _ENTRY[name](*args)
    if rc != 0:
        raise FodError(f"{name} failed ({rc}): {last_error()}")


class Profiler:
    """Optional per-entry-point timing with events on the launching stream (bench.py's roofline leg).

    Disabled (the default) it costs one attribute test per call."""

    def __init__(self):
        self.enabled = False
        self.records = []          # (name, work, start_event, end_event)
        self.pending_work = 0.0

    def start(self):
        self.enabled = True
        self.records = []

    def stop(self):
        self.enabled = False

    def summary(self):
        """{entry: calls, seconds, work, median_us, max_us, outliers (calls > 10 x the entry's median)}: an event pair also
        times whatever stalled the launching thread between its two records while the GPU sat idle, so a host hiccup
        shows up as an outlier here instead of hiding in a sum (BENCH_r02: 24.7 ms booked to a 4.6 ms entry)."""
        import torch
        torch.cuda.synchronize()
        agg = {}
        for name, work, e0, e1 in self.records:
            a = agg.setdefault(name, [[], 0.0])
            a[0].append(e0.elapsed_time(e1) * 1e-3)
            a[1] += work
        out = {}
        for k, (ts, work) in agg.items():
            ts_sorted = sorted(ts)
            med = ts_sorted[len(ts) // 2]
            out[k] = {"calls": len(ts), "seconds": sum(ts), "work": work, "median_us": med * 1e6, "max_us": ts_sorted[-1] * 1e6,
                      "outliers": sum(1 for t in ts if t > 10.0 * med and t > 50e-6)}
        return out


PROFILER = Profiler()


def call(name, *args, work=0.0, tag=None):
    if not PROFILER.enabled:
        return _plain_call(name, *args)
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _plain_call(name, *args)
    e1.record()
    PROFILER.records.append((tag or name, work, e0, e1))
