"""What the host tests read out of the C headers: the text without comments, the struct typedefs, the prototypes reduced to kinds
(i32, u32, i64, u64, f64, i8, ptr, void), and the same reduction of a ctypes type.  Shared by tests/test_host_abi.py and the
per-feature host tests."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC_HEADER = os.path.join(ROOT, "include", "signalalign_hip.h")
IO_HEADER = os.path.join(ROOT, "signalalign_amd", "csrc", "sa_io.h")
INCLUDE_DIRS = [os.path.dirname(PUBLIC_HEADER), os.path.dirname(IO_HEADER)]     # (the Makefile's -I../include -Icsrc)

KIND_OF_C_TYPE = {"void": "void", "char": "i8", "int": "i32", "unsigned": "u32", "unsigned int": "u32", "int32_t": "i32",
                  "uint32_t": "u32", "int64_t": "i64", "uint64_t": "u64", "size_t": "u64", "double": "f64"}


def header_text(path=PUBLIC_HEADER):
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def struct_names(text):
    """every `typedef struct ... { ... } sa_*_t;` that has a body"""
    return re.findall(r"typedef\s+struct\s+\w*\s*\{[^{}]*\}\s*(sa_\w+_t)\s*;", text)


def c_kind(decl):
    """the kind of a parameter declaration (or of a return type); None when it is none of the known ones"""
    if "*" in decl or "[" in decl:
        return "ptr"
    words = [w for w in decl.split() if w != "const"]
    if len(words) > 1 and " ".join(words) not in KIND_OF_C_TYPE:
        words = words[:-1]                                    # the parameter's name
    return KIND_OF_C_TYPE.get(" ".join(words))


def prototypes(text):
    """{function: (kind of the return type, [kind per parameter])} of every sa_* prototype; a declaration that reduces to an
    unknown kind has None in its place"""
    text = text.replace("\\\n", " ")
    text = re.sub(r"#\s*ifdef __cplusplus.*?#\s*endif", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    text = re.sub(r"\{[^{}]*\}", "{};", text)                 # struct bodies; the bodies of the static inline helpers
    out = {}
    for stmt in text.split(";"):
        m = re.fullmatch(r"\s*([\w\s\*]+?)\s*\b(sa_\w+)\s*\((.*)\)\s*", stmt, flags=re.S)
        if not m or m.group(1).split()[0] in ("typedef", "static", "SA_PAIR16_ATTR"):
            continue
        ret, name, params = m.groups()
        params = [p.strip() for p in params.split(",")]
        out[name] = (c_kind(ret + " _"), [] if params == ["void"] or params == [""] else [c_kind(p) for p in params])
    return out


def ctypes_kind(t):
    """the same kinds for a ctypes restype / argtypes entry"""
    if t is None:
        return "void"
    if t in (C.c_char_p, C.c_void_p, C.c_wchar_p) or issubclass(t, (C._Pointer, C.Array)):
        return "ptr"
    if t is C.c_double:
        return "f64"
    code = getattr(t, "_type_", None)
    if code == "c":
        return "i8"
    if isinstance(code, str) and code in "bhilqBHILQ":
        return ("i" if code.islower() else "u") + str(8 * C.sizeof(t))
    return None


def signature_kinds(restype, argtypes):
    return ctypes_kind(restype), [ctypes_kind(a) for a in argtypes]
