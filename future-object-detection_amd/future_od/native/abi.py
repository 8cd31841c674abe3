"""The native ABI as include/fod.h declares it: the one description the ctypes binding (lib.py) and the fast-call
generator (tools/gen_fastcall.py) are built from.  Standard library only; nothing is loaded.

This is a reader of THAT header, not of C: a handful of regular expressions over the comment-stripped text.  Whatever
they do not account for -- a type, a declaration, a macro body -- raises and names it, so a header edit the binding
cannot follow fails at import instead of becoming a wrong argument."""
import ctypes as C
import os
import re


class FodError(RuntimeError):
    pass


HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "..", "include", "fod.h"))
# entry points added without touching fod.h (the header says why); read into tables of their own, see _read_ext()
EXT_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "fod_ext.h")

# kind -> ctypes type.  Every pointer (pointer typedefs and pointers to structs included) travels as a plain address.
CTYPE = {"pointer": C.c_void_p, "int": C.c_int, "long": C.c_long, "float": C.c_float, "size_t": C.c_size_t,
         "unsigned long long": C.c_ulonglong, "uint32_t": C.c_uint32}


def _kind(type_text, pointer_types, where):
    if "*" in type_text:
        return "pointer"
    t = " ".join(w for w in type_text.split() if w != "const")
    if t in pointer_types:
        return "pointer"
    if t in CTYPE:
        return t
    raise FodError(f"fod.h: unknown type '{t}' in '{where}'")


def _value(expr, where):
    """An integer expression of literals, * + << and parentheses; (size_t) casts are dropped."""
    e = expr.replace("(size_t)", "")
    try:
        if not re.fullmatch(r"(?:\d+|<<|[\s()*+])+", e):
            raise SyntaxError(e)
        return int(eval(e, {"__builtins__": {}}))
    except (SyntaxError, TypeError):
        raise FodError(f"fod.h: '{where}' is not an integer expression") from None


_POINTER_TYPEDEF = r"\btypedef\s+struct\s+\w+\s*\*\s*(\w+)\s*;"


def pointer_typedefs(text):
    """The names a header text declares as `typedef struct x* name;` -- what a second header that uses them is read with."""
    return set(re.findall(_POINTER_TYPEDEF, re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)))


def parse(text, pointer_types=()):
    """(prototypes, structs, constants) of a header text (`pointer_types`: pointer typedefs it may use without declaring
    them, i.e. those of a header it includes):
    prototypes: name -> (return kind, [argument kinds]) of every `int|size_t fod_*(...)` declaration, in header order
    structs:    name -> [(field, kind)] of every `typedef struct fod_* {...} fod_*`, in declaration order
    constants:  name -> int for every enumerator of the anonymous enums and every `#define` with an integer body"""
    prototypes, structs, constants, pointer_types = {}, {}, {}, set(pointer_types)
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#\s*ifdef __cplusplus.*?#\s*endif[^\n]*$", "", text, flags=re.S | re.M)    # extern "C" { / }

    def define(m):
        name, body = m.group(1), m.group(2).strip()
        if body:                                                  # (the include guard has none)
            constants[name] = _value(body, f"#define {name} {body}")
        return ""
    text = re.sub(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]*([^\n]*)$", define, text, flags=re.M)
    text = re.sub(r"^[ \t]*#\s*(?:ifndef|endif|include)\b[^\n]*$", "", text, flags=re.M)

    def enum(m):
        nxt = 0
        for item in filter(None, (s.strip() for s in m.group(1).split(","))):
            name, _, expr = (s.strip() for s in item.partition("="))
            if not re.fullmatch(r"\w+", name):
                raise FodError(f"fod.h: enumerator '{item}'")
            constants[name] = nxt = _value(expr, item) if expr else nxt
            nxt += 1
        return ""
    text = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, text)

    def pointer_typedef(m):
        pointer_types.add(m.group(1))
        return ""
    text = re.sub(_POINTER_TYPEDEF, pointer_typedef, text)

    def struct(m):
        name, fields = m.group(1), []
        for decl in filter(None, (" ".join(s.split()) for s in m.group(2).split(";"))):
            first, *more = (s.strip() for s in decl.split(","))
            head = re.fullmatch(r"(.*[\s*])(\w+)", first)
            if not head or ("*" in decl and more) or not all(re.fullmatch(r"\w+", s) for s in more):
                raise FodError(f"fod.h: field '{decl}' of {name}")
            kind = _kind(head.group(1), pointer_types, f"{decl} (struct {name})")
            fields += [(f, kind) for f in [head.group(2)] + more]
        structs[name] = fields
        return ""
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;", struct, text)

    def prototype(m):
        ret, name, params = m.group(1), m.group(2), " ".join(m.group(3).split())
        args = []
        if params != "void":
            for p in (s.strip() for s in params.split(",")):
                head = re.fullmatch(r"(.*[\s*])(\w+)", p)
                if not head:
                    raise FodError(f"fod.h: parameter '{p}' of {name}")
                args.append(_kind(head.group(1), pointer_types, f"{p} ({name})"))
        prototypes[name] = (ret, args)
        return ""
    text = re.sub(r"\b(int|size_t)\s+(fod_\w+)\s*\(([^()]*)\)\s*;", prototype, text)

    if text.strip():
        raise FodError(f"fod.h: cannot read '{text.strip().splitlines()[0].strip()}'")
    return prototypes, structs, constants


def served(prototypes):
    """name -> [argument kinds] of the entry points lib.call() and the fast-call wrappers serve: the prototypes that
    return int, less the two plain getters the binding reads directly."""
    return {name: args for name, (ret, args) in prototypes.items()
            if ret == "int" and name not in ("fod_abi_version", "fod_multi_chunk")}


def det_twins(prototypes):
    """{entry point: its `_det` twin takes (scratch, bytes) in front of the stream} for every pair x / x_det that a
    caller may swap by the header's rule: the twin's arguments are x's plus `void* ws, size_t ws_bytes` in front of the
    stream -- or x's own where x takes such a scratch already (False).  Any other pair raises."""
    same_arguments = ("fod_gemm_tn_acc", "fod_conv2d_wgrad_acc")      # their (optional) workspace becomes the scratch
    own_form = ("fod_gemm_tn_multi_long",)      # the twin also takes its table's scratch offsets: not swapped blindly
    twins = {}
    for det, (ret, args) in prototypes.items():
        name = det[:-4]
        if not det.endswith("_det") or name not in prototypes:
            continue
        base = prototypes[name][1]
        if name in own_form and args[:len(base) - 1] + args[-3:] == base[:-1] + ["pointer", "size_t"] + base[-1:]:
            continue
        if (ret, args) == (prototypes[name][0], base[:-1] + ["pointer", "size_t"] + base[-1:]):
            twins[name] = True
        elif name in same_arguments and (ret, args) == prototypes[name] and args[-3:-1] == ["pointer", "size_t"]:
            twins[name] = False
        else:
            raise FodError(f"fod.h: {det} is not {name} plus (void* ws, size_t ws_bytes) in front of the stream")
    return twins


def _read():
    if not os.path.isfile(HEADER_PATH):
        raise FodError(f"{HEADER_PATH} not found: the binding is built from the header, there is no second copy")
    with open(HEADER_PATH) as f:
        return parse(f.read())


def _read_ext():
    """The prototypes of include/fod_ext.h, read with fod.h's pointer typedefs.  It adds entry points and nothing else:
    a struct, a constant or a name fod.h has is refused."""
    for path in (HEADER_PATH, EXT_HEADER_PATH):
        if not os.path.isfile(path):
            raise FodError(f"{path} not found: the binding is built from the header, there is no second copy")
    with open(HEADER_PATH) as f:
        known = pointer_typedefs(f.read())
    with open(EXT_HEADER_PATH) as f:
        prototypes, structs, constants = parse(f.read(), known)
    extra = sorted(structs) + sorted(constants) + sorted(set(prototypes) & set(PROTOTYPES))
    if extra:
        raise FodError(f"fod_ext.h declares {', '.join(extra)}: it holds new prototypes only")
    return prototypes


PROTOTYPES, STRUCTS, CONSTANTS = _read()
EXT_PROTOTYPES = _read_ext()
