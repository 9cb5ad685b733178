"""The ctypes binding against the two headers, on the CPU: what Python passes is what C expects, for every function and every
struct. plbert_amd/_lib.py holds one table per header (name -> (restype, [argtypes])) and declare() applies them; here
 - every prototype of include/plbert.h and csrc/plbert_kernels.h has a table entry and nothing else has (two independent
   extractions of the names have to agree),
 - every entry follows the type rules (width and signedness, POINTER(struct) for a mirrored struct),
 - every ctypes.Structure mirror has the layout a C++ compiler gives the header's struct,
 - declare() works symbol by symbol, so a library that predates a feature is fully declared in what it has,
 - every plb_* symbol the built library exports is declared, and nobody else assigns argtypes / restype."""
import ctypes as C
import glob
import inspect
import os
import re
import shutil
import subprocess

import pytest

import c_header
from plbert_amd import _lib

ROOT = c_header.ROOT
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HEADERS = {"public": (c_header.public, _lib.PUBLIC), "kernels": (c_header.kernels, _lib.INTERNAL)}
MIRRORS = {n: v for n, v in vars(_lib).items() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}
TABLE = {**_lib.PUBLIC, **_lib.INTERNAL}


@pytest.mark.parametrize("which", sorted(HEADERS))
def test_every_prototype_is_bound_and_only_prototypes_are(which):
    parse, table = HEADERS[which]
    hdr = parse()
    loose = set(re.findall(r"\b(plb_[a-z_0-9]+)\s*\(", hdr.text)) - set(hdr.inline)   # test_cabi_and_host._declared_symbols
    assert len(hdr.protos) >= 60, sorted(hdr.protos)
    assert set(hdr.protos) == loose, f"the parser and the loose scan disagree on {sorted(set(hdr.protos) ^ loose)}"
    assert set(table) == set(hdr.protos), (f"prototypes without a table entry: {sorted(set(hdr.protos) - set(table))}; "
                                           f"entries without a prototype: {sorted(set(table) - set(hdr.protos))}")
    if which == "public":
        assert _lib.PUBLIC_SYMBOLS == list(_lib.PUBLIC)


def test_a_name_in_both_tables_has_one_signature():
    for name in set(_lib.PUBLIC) & set(_lib.INTERNAL):
        assert _lib.PUBLIC[name] == _lib.INTERNAL[name], name


@pytest.mark.parametrize("which", sorted(HEADERS))
def test_every_signature_follows_the_type_rules(which):
    parse, table = HEADERS[which]
    hdr = parse()
    wrong = [c_header.signature_mismatch(hdr, p, *table[name], MIRRORS) for name, p in hdr.protos.items() if name in table]
    assert not any(wrong), "\n".join(w for w in wrong if w)


def _header_structs():
    out = {}
    for parse, _ in HEADERS.values():
        hdr = parse()
        out.update({name: (hdr, fields) for name, fields in hdr.structs.items()})
    return out


def _compiler():
    for cand in (os.path.join(ROCM, "lib", "llvm", "bin", "clang++"), shutil.which("g++")):
        if cand and os.path.exists(cand):
            return cand
    raise AssertionError("no C++ compiler: neither ROCm's clang++ nor g++")


def test_every_struct_mirror_has_the_compilers_layout(tmp_path):
    structs = _header_structs()
    assert len(MIRRORS) >= 7 and set(MIRRORS) <= set(structs), f"mirrors of no header struct: {sorted(set(MIRRORS) - set(structs))}"
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "plbert_kernels.h"', '#include "plbert.h"', "int main() {"]
    for name in MIRRORS:
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for f in structs[name][1]:
            lines.append(f'  printf("{name}.{f.name} %zu %zu\\n", offsetof({name}, {f.name}), sizeof((({name}*)0)->{f.name}));')
    lines += ["  return 0;", "}", ""]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines))
    cmd = [_compiler(), "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include", "-I", os.path.join(ROOT, "plbert_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    sizes, fields = {}, {n: [] for n in MIRRORS}
    for ln in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines():
        what, *nums = ln.split()
        if "." in what:
            fields[what.split(".")[0]].append((what.split(".")[1], int(nums[0]), int(nums[1])))
        else:
            sizes[what] = int(nums[0])
    for name, cls in MIRRORS.items():
        mine = [(f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_]
        diff = [(a, b) for a, b in zip(mine, fields[name]) if a != b]
        assert not diff, f"{name}: field (name, offset, size) {diff[0][0]} in _lib, {diff[0][1]} in the header"
        assert len(mine) == len(fields[name]), f"{name}: {len(mine)} fields in _lib, {len(fields[name])} in the header"
        assert C.sizeof(cls) == sizes[name], f"{name}: sizeof {C.sizeof(cls)} in _lib, {sizes[name]} in the header"


def test_every_struct_mirror_field_has_the_headers_type():
    """The layout cannot tell a float from an int32: a scalar field is the ctypes type of its C type, a pointer c_void_p."""
    for name, (hdr, fields) in _header_structs().items():
        if name in MIRRORS:
            for f, (fname, ftype) in zip(fields, MIRRORS[name]._fields_):
                want = C.c_void_p if f.depth else hdr.scalar(f.base)
                assert fname == f.name and ftype is want, f"{name}.{f.name}: `{f.text}` is mirrored as ({fname}, {ftype})"


class _Fn:
    restype = argtypes = "undeclared"


class _StandIn:
    def __init__(self, names):
        for n in names:
            setattr(self, n, _Fn())


_ALL = sorted(TABLE)
_PACKED_DUAL = ("plb_loss_fwd_bwd_dual_packed", "plb_launch_pack_token_targets", "plb_launch_token_ce_combine_packed")
SUBSETS = {
    "all": _ALL, "none": [], "public": list(_lib.PUBLIC), "every other": _ALL[::2], "one": ["plb_launch_adamw"],
    # a library that has packed dual-head calls and predates plb_set_packed_fp8 (and the features after it)
    "before packed fp8": [n for n in _ALL if n not in ("plb_set_packed_fp8", "plb_grad_accum_add", "plb_launch_grad_accum")],
}


@pytest.mark.parametrize("subset", sorted(SUBSETS))
def test_declare_is_per_symbol(subset):
    names = SUBSETS[subset]
    L = _StandIn(names)
    assert _lib.declare(L) is L
    assert sorted(vars(L)) == sorted(names)                 # absent symbols are not created
    for n in names:
        fn = getattr(L, n)
        assert (fn.restype, fn.argtypes) == TABLE[n], n
    if subset == "before packed fp8":
        assert not hasattr(L, "plb_set_packed_fp8")
        for n in _PACKED_DUAL:
            assert getattr(L, n).argtypes == TABLE[n][1] and len(TABLE[n][1]) >= 8, n


def test_nothing_the_library_exports_is_undeclared():
    readelf = os.path.join(ROCM, "lib", "llvm", "bin", "llvm-readelf")
    assert os.path.exists(readelf), readelf
    _lib.lib()   # (the in-tree build for gfx950; raises when it is missing)
    out = subprocess.run([readelf, "--dyn-syms", "--wide", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set()
    for ln in out.splitlines():
        col = ln.split()
        if len(col) == 8 and col[6] != "UND" and col[7].startswith("plb_"):
            exported.add(col[7].split("@")[0])
    assert len(exported) >= 100, sorted(exported)
    assert not exported - set(TABLE), f"exported and undeclared: {sorted(exported - set(TABLE))}"


def test_no_stray_declarations():
    """argtypes / restype are assigned in _lib.declare and nowhere else (the stand-in RCCL library's own fake_rccl_* symbols
    are not this ABI)."""
    src, first = inspect.getsourcelines(_lib.declare)
    allowed = {(os.path.join("plbert_amd", "_lib.py"), first + k) for k in range(len(src))}
    files = [os.path.join(ROOT, "bench.py")]
    for d in ("tests", "tools", "plbert_amd"):
        files += glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True)
    stray = []
    for path in files:
        rel = os.path.relpath(path, ROOT)
        for no, ln in enumerate(open(path), 1):
            if re.search(r"\.(argtypes|restype)\b\s*(,[^=\n]*)?=(?!=)", ln) and "fake_rccl_" not in ln and (rel, no) not in allowed:
                stray.append(f"{rel}:{no}: {ln.strip()}")
    assert len(files) > 60 and not stray, "\n".join(stray)
