"""The binding is built from include/fod.h (future_od/native/abi.py): the header reader on small header texts, the
ctypes struct layouts against what the C compiler lays out, the whole tables against the built library, and the rule
that lets a caller swap an entry point for its `_det` twin."""
import ctypes
import os
import shutil
import subprocess

import pytest

from future_od.native import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, L_, F, Z = "pointer", "int", "long", "float", "size_t"


def test_reader_prototypes_comments_lines_and_scalar_kinds():
    protos, structs, consts = abi.parse("""
        /* a comment that says: int fod_not_this(int x); */
        #ifndef FOD_H_
        #define FOD_H_
        #include <stddef.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        typedef struct ihipStream_t* fod_stream_t; /* == hipStream_t */
        int fod_a(int dtype, const void* G, long ldg, float* dW,
                  void* ws /* optional, FOD_TN_WS_BYTES: partial tiles */,
                  size_t ws_bytes, fod_stream_t stream);
        int fod_b(const fod_thing* epi,
                  /* res_nseg > 0: the residual is res_nseg blocks,
                   * 0: one residual */
                  int res_nseg, long res_seg_stride, fod_stream_t stream);   // trailing
        int fod_c(void);
        int fod_d(int njobs, const void* const* ptrs, const int64_t* labels, char* out, void** flag);
        int fod_e(unsigned long long seed, const unsigned long long* seed_dev, uint32_t ticket, size_t n, float p);
        size_t fod_f(char* buf, size_t cap);
        #ifdef __cplusplus
        }
        #endif
        #endif /* FOD_H_ */
    """)
    assert protos == {
        "fod_a": (I, [I, P, L_, P, P, Z, P]),
        "fod_b": (I, [P, I, L_, P]),
        "fod_c": (I, []),
        "fod_d": (I, [I, P, P, P, P]),
        "fod_e": (I, ["unsigned long long", P, "uint32_t", Z, F]),
        "fod_f": (Z, [P, Z]),
    }
    assert list(protos) == ["fod_a", "fod_b", "fod_c", "fod_d", "fod_e", "fod_f"]       # header order
    assert structs == {} and consts == {}                                               # the include guard is no constant
    assert [abi.CTYPE[k] for k in protos["fod_e"][1]] == [ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_uint32,
                                                          ctypes.c_size_t, ctypes.c_float]


def test_reader_structs_with_several_declarators():
    _, structs, _ = abi.parse("""
        typedef struct fod_s {
          const void* G;
          float* dW;
          long ldg, ldx, ldw;   /* three in one declaration */
          int B, H, Tq, S;
          float scale;
          unsigned long long drop_seed;
          const unsigned long long* drop_seed_dev;
          int m_per_split, nsplit;   /* a comment; with a semicolon */
        } fod_s;
    """)
    assert structs == {"fod_s": [("G", P), ("dW", P), ("ldg", L_), ("ldx", L_), ("ldw", L_), ("B", I), ("H", I), ("Tq", I),
                                 ("S", I), ("scale", F), ("drop_seed", "unsigned long long"), ("drop_seed_dev", P),
                                 ("m_per_split", I), ("nsplit", I)]}


def test_reader_enumerators_and_macro_bodies():
    _, _, consts = abi.parse("""
        enum { FOD_F32 = 0, FOD_BF16 = 1 };
        enum { FOD_A, FOD_B, FOD_C = 7, FOD_D,   /* implicit values count on */
               FOD_E = 2 };
        enum {
          FOD_EW_ADD = 0,       /* out = a + b */
          FOD_EW_MUL = 1        /* out = a * b */
        };
        #define FOD_ABI_VERSION 9
        #define FOD_TN_WS_BYTES ((size_t)64 << 20)
        #define FOD_PER_TILE (8 * 2176)
        #define FOD_FLOATS (64 * 8 * 4096)
        #define FOD_SUM (1 + 2 * 3)
    """)
    assert consts == {"FOD_F32": 0, "FOD_BF16": 1, "FOD_A": 0, "FOD_B": 1, "FOD_C": 7, "FOD_D": 8, "FOD_E": 2,
                      "FOD_EW_ADD": 0, "FOD_EW_MUL": 1, "FOD_ABI_VERSION": 9, "FOD_TN_WS_BYTES": 64 << 20,
                      "FOD_PER_TILE": 8 * 2176, "FOD_FLOATS": 64 * 8 * 4096, "FOD_SUM": 7}
    assert all(type(v) is int for v in consts.values())


@pytest.mark.parametrize("text,names", [
    ("int fod_x(int a, double x);", ("double", "fod_x")),                          # a type the reader does not know
    ("typedef struct fod_e { int a; } fod_e;\nint fod_y(fod_e epi, int n);", ("fod_e epi", "fod_y")),     # struct by value
    ("typedef struct fod_s { double d; } fod_s;", ("double", "fod_s")),
    ("typedef struct fod_s { int *a, b; } fod_s;", ("int *a, b", "fod_s")),
    ("typedef struct fod_s { int a; } fod_t;", ("fod_s", "fod_t")),
    ("const char* fod_name(int code);", ("fod_name",)),                            # a return type it does not know
    ("void fod_reset(void);", ("fod_reset",)),
    ("int fod_cb(int (*fn)(int), int n);", ("fod_cb",)),
    ("int fod_z(int);", ("fod_z",)),                                               # no parameter name: cannot tell
    ("#define FOD_NAME \"text\"", ("FOD_NAME",)),
    ("#define FOD_MAX(a, b) ((a) > (b) ? (a) : (b))", ("FOD_MAX",)),
    ("#define FOD_CMP (1 < 2)", ("FOD_CMP",)),
    ("enum { FOD_NEG = -1 };", ("FOD_NEG",)),
    ("enum fod_kind { FOD_K0 };", ("fod_kind",)),
])
def test_reader_raises_and_names_what_it_does_not_know(text, names):
    with pytest.raises(abi.FodError) as e:
        abi.parse(text)
    for name in names:
        assert name in str(e.value), (name, str(e.value))


def test_a_missing_header_is_an_error_with_its_path(monkeypatch, tmp_path):
    gone = str(tmp_path / "include" / "fod.h")
    monkeypatch.setattr(abi, "HEADER_PATH", gone)
    with pytest.raises(abi.FodError, match="fod.h not found") as e:
        abi._read()
    assert gone in str(e.value)


def test_the_header_reads_whole():
    """What the tables must contain today (ABI 9); the same header that every other test of this file compares with."""
    assert os.path.samefile(abi.HEADER_PATH, os.path.join(ROOT, "include", "fod.h"))
    assert len(abi.PROTOTYPES) == 86 and len(abi.STRUCTS) == 8 and len(abi.served(abi.PROTOTYPES)) == 82
    assert [n for n, (ret, _) in abi.PROTOTYPES.items() if ret == "size_t"] == ["fod_last_error", "fod_workspace_bytes"]
    # comments inside the parameter lists
    assert abi.PROTOTYPES["fod_gemm_tn_acc"] == (I, [I, P, L_, P, L_, P, L_, I, I, I, P, P, I, P, Z, P])
    assert abi.PROTOTYPES["fod_gemm_nt_grouped"][1][-4:] == [P, I, L_, P]
    assert abi.PROTOTYPES["fod_linear_add_norm_fwd"][1][-5:] == [F, P, P, P, P]
    assert abi.PROTOTYPES["fod_attn_bwd_dkv_multi"] == (I, [I, I, P, P, P])
    assert abi.PROTOTYPES["fod_abi_version"] == (I, [])
    assert abi.STRUCTS["fod_attn_shape"][:5] == [("B", I), ("H", I), ("Tq", I), ("S", I), ("q_batch_stride", L_)]
    assert abi.CONSTANTS["FOD_WS_TN_MULTI_DET"] == 5 and abi.CONSTANTS["FOD_EW_COPY_B"] == 6
    assert abi.CONSTANTS["FOD_NT_SPLIT_WS_FLOATS"] == 64 * 8 * 4096 and "FOD_H_" not in abi.CONSTANTS


def test_binding_tables_are_the_headers():
    from future_od.native import lib as L
    from future_od.native import ops
    assert L.FodError is abi.FodError
    assert L.EXPORTS == sorted(abi.PROTOTYPES)
    assert set(L.SIGNATURES) == set(L.EXPORTS) - {"fod_last_error", "fod_workspace_bytes", "fod_abi_version", "fod_multi_chunk"}
    for name, sig in L.SIGNATURES.items():
        assert sig == [abi.CTYPE[k] for k in abi.PROTOTYPES[name][1]], name
    for name, (ret, args) in abi.PROTOTYPES.items():
        fn = getattr(L.LIB, name)                                   # every prototype is exported by the built library
        assert fn.restype is abi.CTYPE[ret] and list(fn.argtypes) == [abi.CTYPE[k] for k in args], name
    assert L.LIB.fod_abi_version() == abi.CONSTANTS["FOD_ABI_VERSION"] == L.ABI_VERSION
    want = {"FOD_WS_NT_SPLIT": abi.CONSTANTS["FOD_NT_SPLIT_WS_FLOATS"] * 4,
            "FOD_WS_NT_SPLIT_TICKETS": abi.CONSTANTS["FOD_NT_SPLIT_TICKETS"] * 4,
            "FOD_WS_TN_PARTIALS": abi.CONSTANTS["FOD_TN_WS_BYTES"],
            "FOD_WS_ATTN_SPLIT_PER_TILE": abi.CONSTANTS["FOD_ATTN_SPLIT_WS_FLOATS_PER_TILE"] * 4,
            "FOD_WS_DET": abi.CONSTANTS["FOD_DET_WS_BYTES"],
            "FOD_WS_TN_MULTI_DET": abi.CONSTANTS["FOD_TN_MULTI_DET_WS_BYTES"]}
    assert set(want) == {k for k in abi.CONSTANTS if k.startswith("FOD_WS_")}          # every kind the header lists
    for kind, nbytes in want.items():
        assert L.LIB.fod_workspace_bytes(abi.CONSTANTS[kind]) == nbytes > 0, kind
    # the public constants are the header's, under their names without FOD_ / ROUTE_
    for c_name, name in (("FOD_F32", "F32"), ("FOD_BF16", "BF16"), ("FOD_EW_RELU_MASK", "EW_RELU_MASK"),
                         ("FOD_ROUTE_NT_BIG", "NT_BIG"), ("FOD_ROUTE_TN_128", "TN_128"), ("FOD_CONV_WGRAD", "CONV_WGRAD"),
                         ("FOD_ATTN_PREFETCH", "ATTN_PREFETCH"), ("FOD_WS_DET", "WS_DET"),
                         ("FOD_TN_DET_MAX_SPLITS", "TN_DET_MAX_SPLITS"),
                         ("FOD_ATTN_SPLIT_WS_FLOATS_PER_TILE", "ATTN_SPLIT_WS_FLOATS_PER_TILE")):
        assert getattr(L, name) == abi.CONSTANTS[c_name] and type(getattr(L, name)) is int, name
    assert ops._DET_TWINS == abi.det_twins(abi.PROTOTYPES)


STRUCT_CLASSES = {"fod_epilogue": "Epilogue", "fod_conv_geom": "ConvGeom", "fod_attn_shape": "AttnShape",
                  "fod_permute_job": "PermuteJob", "fod_tn_job": "TnJob", "fod_nt_route": "NtRoute",
                  "fod_tn_route": "TnRoute", "fod_attn_kernels": "AttnRoute"}


def test_struct_layouts_are_the_compilers(tmp_path):
    """sizeof / offsetof of every struct and field of the header, printed by a C program the host compiler builds from
    include/fod.h, against the ctypes classes."""
    from future_od.native import lib as L
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler on PATH")
    assert set(STRUCT_CLASSES) == set(abi.STRUCTS)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "fod.h"', 'int main(void) {']
    for name, fields in abi.STRUCTS.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for field, _ in fields:
            lines.append(f'  printf("{name}.{field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name}*)0)->{field}));')
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout
    got = {w[0]: tuple(int(v) for v in w[1:]) for w in (line.split() for line in out.splitlines())}
    want = {}
    for name, fields in abi.STRUCTS.items():
        cls = getattr(L, STRUCT_CLASSES[name])
        assert [f for f, _ in cls._fields_] == [f for f, _ in fields], name
        want[name] = (ctypes.sizeof(cls),)
        for (field, ctype), _ in zip(cls._fields_, fields):
            want[f"{name}.{field}"] = (getattr(cls, field).offset, ctypes.sizeof(ctype))
    assert len(want) == len(abi.STRUCTS) + sum(len(f) for f in abi.STRUCTS.values()) == 8 + 97
    assert got == want, sorted(set(got.items()) ^ set(want.items()))


TWIN_HEADER = """
    typedef struct ihipStream_t* fod_stream_t;
    int fod_sum(int dtype, const void* g, float* out, fod_stream_t stream);
    int fod_sum_det(int dtype, const void* g, float* out, %s fod_stream_t stream);
    int fod_gemm_tn_acc(int dtype, const void* g, void* ws, size_t ws_bytes, fod_stream_t stream);
    int fod_gemm_tn_acc_det(int dtype, const void* g, void* ws, size_t ws_bytes, fod_stream_t stream);
    int fod_gemm_tn_multi_long(const void* jobs, int nblocks, fod_stream_t stream);
    int fod_gemm_tn_multi_long_det(const void* jobs, int nblocks, const long* part_off, int njobs, void* ws,
                                   size_t ws_bytes, fod_stream_t stream);
    int fod_multi_sqnorm_det(const long* ptrs, float* out, float* scratch, fod_stream_t stream);   /* no fod_multi_sqnorm */
"""


def test_det_twin_rule():
    good = abi.parse(TWIN_HEADER % "void* ws, size_t ws_bytes,")[0]
    assert abi.det_twins(good) == {"fod_sum": True, "fod_gemm_tn_acc": False}
    assert abi.det_twins(abi.PROTOTYPES) == {
        "fod_gemm_tn_acc": False, "fod_conv2d_wgrad_acc": False, "fod_colsum_acc": True, "fod_layernorm_bwd": True,
        "fod_linear_add_norm_bwd": True, "fod_mlp2_mul_bwd": True}
    for wrong in ("size_t ws_bytes, void* ws,",              # the pair the other way round
                  "void* ws, long ws_bytes,",                # the size as another type
                  "void* ws,",                               # no size
                  "",                                        # the same arguments, but not one of the two stated entries
                  "int extra, void* ws, size_t ws_bytes,"):
        with pytest.raises(abi.FodError, match="fod_sum_det is not fod_sum plus"):
            abi.det_twins(abi.parse(TWIN_HEADER % wrong)[0])
    swapped = dict(good, fod_sum_det=(I, [P, I, P, P, Z, P]))         # an int and a pointer changed places
    with pytest.raises(abi.FodError, match="fod_sum_det"):
        abi.det_twins(swapped)
    moved = dict(good, fod_gemm_tn_multi_long_det=(I, [P, I, P, I, P, P, Z]))      # scratch not in front of the stream
    with pytest.raises(abi.FodError, match="fod_gemm_tn_multi_long_det"):
        abi.det_twins(moved)
