"""A parser of the C declarations in include/plbert.h and plbert_amd/csrc/plbert_kernels.h, for the host tests that hold the
ctypes binding (plbert_amd/_lib.py) to the headers. It knows what those two files contain: prototypes with multi-line
parameter lists, `const T* const*`, array parameters, `typedef struct { ... } Name;` with comma declarators that carry their
own stars (`float *mean, *rstd;`, `int B, S, NH, H;`), enums, plain typedefs, `static inline` definitions and macros."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC_HEADER = os.path.join(ROOT, "include", "plbert.h")
KERNEL_HEADER = os.path.join(ROOT, "plbert_amd", "csrc", "plbert_kernels.h")

SCALARS = {
    "int": C.c_int32, "int32_t": C.c_int32, "unsigned int": C.c_uint32, "uint32_t": C.c_uint32,
    "int64_t": C.c_int64, "uint64_t": C.c_uint64, "unsigned long long": C.c_uint64, "size_t": C.c_size_t,
    "float": C.c_float, "double": C.c_double, "int8_t": C.c_int8, "uint8_t": C.c_uint8, "uint16_t": C.c_uint16,
    "char": C.c_char,
}
HANDLES = ("hipStream_t",)   # opaque pointers passed by value


def strip_comments(text):
    """The text without /* */ and // comments (neither header has a string literal that holds one)."""
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


class Decl:
    """One parameter or struct field: `base` without qualifiers ("float", "PlbGemmNT", "void"), the pointer depth (an array
    parameter counts as one level) and the name."""

    def __init__(self, base, depth, name, text):
        self.base, self.depth, self.name, self.text = base, depth, name, text

    def __repr__(self):
        return f"{self.base}{'*' * self.depth} {self.name}"


class Proto:
    def __init__(self, name, ret, params):
        self.name, self.ret, self.params = name, ret, params

    @property
    def texts(self):
        """The parameters as written, white space normalised: ["PlbEngine* e", "int32_t on"]."""
        return [p.text for p in self.params]


class Header:
    def __init__(self, path):
        self.path = path
        self.text = strip_comments(open(path).read())
        self.protos, self.structs, self.aliases, self.inline = {}, {}, {}, []
        for st in _statements(self.text):
            self._statement(st)

    def _statement(self, st):
        body = re.match(r"typedef\s+struct\s*\{(.*)\}\s*(\w+)$", st, re.S)
        if body:
            self.structs[body.group(2)] = _fields(body.group(1))
        elif st.startswith("enum") or re.match(r"typedef\s+struct\s+\w+\s+\w+$", st):
            pass
        elif st.startswith("typedef"):
            words = st.split()
            self.aliases[words[-1]] = " ".join(words[1:-1])
        elif "{" in st:                        # a definition: the headers have `static inline` ones only
            assert st.startswith("static inline"), st
            self.inline.append(re.match(r"[^(]*?(\w+)\s*\(", st).group(1))
        else:
            m = re.match(r"(.*?)(\w+)\s*\((.*)\)$", st, re.S)
            assert m, f"{self.path}: cannot parse {st!r}"
            ret = _declarator(m.group(1) + " _")
            params = [] if m.group(3).strip() == "void" else [_declarator(p) for p in m.group(3).split(",")]
            assert m.group(2) not in self.protos or self.protos[m.group(2)].texts == [p.text for p in params], m.group(2)
            self.protos[m.group(2)] = Proto(m.group(2), ret, params)

    def scalar(self, base):
        """The ctypes type of a scalar base type (typedefs of the header resolved), or None for void / structs."""
        return SCALARS.get(self.aliases.get(base, base))


def _statements(text):
    """Top-level statements, without preprocessor lines and the `extern "C" { }` wrapper: each ends at its `;`, a function
    definition at the brace that closes its body."""
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', "", text)
    cur, depth = [], 0
    for ch in text:
        if ch == "}" and depth == 0:           # the wrapper's closing brace
            continue
        if ch == ";" and depth == 0:
            yield " ".join("".join(cur).split())
            cur = []
            continue
        cur.append(ch)
        depth += (ch == "{") - (ch == "}")
        if ch == "}" and depth == 0 and "(" in "".join(cur).split("{", 1)[0]:
            yield " ".join("".join(cur).split())
            cur = []
    assert depth == 0 and not "".join(cur).strip(), "".join(cur)[-200:]


def _declarator(piece, base=None):
    """`const bf16_t* A`, `float clamped_calls[8]`, `const void* const* src`; with `base`: one name of a comma list."""
    text = " ".join(piece.split())
    depth = piece.count("*") + piece.count("[")
    words = [w for w in re.findall(r"[A-Za-z_]\w*", re.sub(r"\[[^\]]*\]", "", piece)) if w != "const"]
    assert words, piece
    if base is None:
        assert len(words) >= 2, piece
        base = " ".join(words[:-1])
    else:
        assert len(words) == 1, piece
    return Decl(base, depth, words[-1], text)


def _fields(body):
    out = []
    for st in body.split(";"):
        if not st.strip():
            continue
        pieces = st.split(",")
        first = _declarator(pieces[0])
        out.append(first)
        out.extend(_declarator(p, first.base) for p in pieces[1:])
    return out


def public():
    return Header(PUBLIC_HEADER)


def kernels():
    return Header(KERNEL_HEADER)


def _is_pointer_type(t):
    return isinstance(t, type) and issubclass(t, C._Pointer)


def signature_mismatch(header, proto, restype, argtypes, mirrors):
    """None when (restype, argtypes) is what the binding's type rules give for `proto`, else a text that names the function
    and the parameter. The rules (plbert_amd/_lib.py): a scalar maps to the ctypes type of its width and signedness; a
    pointer to a struct that `mirrors` ({name: ctypes.Structure}) holds must be POINTER(that class); any other pointer, an
    array parameter and a stream are c_void_p, or POINTER(the pointee's own type); `const char*` returns c_char_p, void None."""
    ret = proto.ret
    want = None if (ret.base, ret.depth) == ("void", 0) else C.c_char_p if (ret.base, ret.depth) == ("char", 1) \
        else header.scalar(ret.base) if ret.depth == 0 else C.c_void_p
    if restype is not want:
        return f"{proto.name}: returns {ret.text[:-2]}, restype is {restype} instead of {want}"
    if len(argtypes) != len(proto.params):
        return f"{proto.name}: {len(proto.params)} parameters, {len(argtypes)} argtypes"
    for k, (d, t) in enumerate(zip(proto.params, argtypes)):
        if d.depth == 0 and d.base not in HANDLES:
            ok, want = t is header.scalar(d.base) and t is not None, header.scalar(d.base)
        elif d.depth == 0:
            ok, want = t is C.c_void_p, C.c_void_p
        elif d.depth == 1 and d.base in mirrors:
            ok, want = t is C.POINTER(mirrors[d.base]), f"POINTER({d.base})"
        else:
            pointee = C.c_void_p if d.depth > 1 else header.scalar(d.base)
            ok = t is C.c_void_p or (pointee is not None and _is_pointer_type(t) and t._type_ is pointee)
            want = f"c_void_p or POINTER({pointee})"
        if not ok:
            return f"{proto.name}: parameter {k} `{d.text}` is bound as {t}, the rules give {want}"
    return None


def mirrors(module):
    """{name: class} of the ctypes.Structure classes a binding module defines."""
    return {n: v for n, v in vars(module).items() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}


def bound_mismatch(header, fn, module):
    """signature_mismatch for a function of a loaded library as `module` declared it."""
    return signature_mismatch(header, header.protos[fn.__name__], fn.restype, fn.argtypes, mirrors(module))


def c_params(header, name):
    """The parameter texts of one `int name(...)` prototype (what the per-feature tests compare names and positions on)."""
    proto = header.protos[name]
    assert proto.ret.base == "int" and proto.ret.depth == 0, name
    return proto.texts
