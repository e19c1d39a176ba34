"""The one reader of the C headers under include/ for the ABI tests (tests/test_abi_headers.py), and the fake pointer and the 16-byte
round-up the argument-check tests share.  A header is read once, comments stripped; a declaration belongs to the file that spells it, so
what `#include "other.h"` brings in is other.h's."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess
import tempfile
from typing import NamedTuple

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
FAKE = 0x10000             # a non-NULL, 16-byte aligned "pointer": a call given it must fail before anything dereferences it


def fake(offset=0):
    return FAKE + offset


def a16(n):
    return (n + 15) & ~15


class Parsed(NamedTuple):
    text: str              # the file without its comments
    includes: tuple        # the project headers it includes
    functions: tuple       # declared function names, in order
    structs: dict          # tag -> [(C type, field, array length | None)], `typedef struct tag { ... } tag_t;`
    constants: dict        # `#define NAME <int>` and enumerators `NAME = <int>`


_SCALARS = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}


@functools.lru_cache(maxsize=None)
def read(name) -> Parsed:
    with open(os.path.join(INCLUDE, name)) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    constants = {k: int(v) for k, v in re.findall(r"^[ \t]*#define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$", text, re.M)}
    for body in re.findall(r"\benum\s*\{(.*?)\}", text, re.S):
        for item in filter(None, (i.strip() for i in body.split(","))):
            k, v = re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", item).groups()          # every enumerator of these headers states its value
            assert k not in constants, (name, k)
            constants[k] = int(v)
    structs = {}
    for tag, body, alias in re.findall(r"\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, re.S):
        assert alias == tag + "_t" and tag not in structs, (name, tag, alias)
        fields = structs[tag] = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            first, *more = (d.strip() for d in decl.split(","))
            base, star, field, length = re.fullmatch(r"(.*?)\s*(\**)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?", first).groups()
            fields.append((base + star, field, length))
            for d in more:                                                      # `int32_t B, C, H, W;`: a later declarator repeats the base type
                star, field, length = re.fullmatch(r"(\**)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?", d).groups()
                fields.append((base + star, field, length))
    rest = re.sub(r"\b(typedef\s+struct|enum)\b[^{;]*\{.*?\}[^;]*;", " ", text, flags=re.S)
    rest = re.sub(r"^[ \t]*#.*$", " ", rest, flags=re.M)
    functions = tuple(re.findall(r"\b(\w+)\s*\(", rest))
    assert len(functions) == len(set(functions)), (name, functions)
    return Parsed(text, tuple(re.findall(r'^[ \t]*#include[ \t]+"(\w+\.h)"', text, re.M)), functions, structs, constants)


def headers():
    return sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h"))


def visible_constants(name) -> dict:
    """The constants a header sees: its own and those of the headers it includes, as the preprocessor would resolve them"""
    out = {}
    for inc in read(name).includes:
        out.update(visible_constants(inc))
    out.update(read(name).constants)
    return out


def header_of(tag):
    (name,) = [h for h in headers() if tag in read(h).structs]
    return name


def array_length(name, length):
    """A field's array length as an int: None (no array), a literal, or one of the header's macros"""
    if length is None:
        return None
    return int(length) if length.isdigit() else visible_constants(name)[length]


@functools.lru_cache(maxsize=None)
def ctypes_from_header(tag):
    """A ctypes Structure built from the C types the header spells -- the layout the C rules give them, with no compiler and no mirror
    involved: every pointer is a c_void_p, `<tag>_t` is that struct by value, `name[N]` an array of N (a literal or a macro)."""
    name = header_of(tag)
    fields = []
    for ctype, field, length in read(name).structs[tag]:
        ctype = re.sub(r"\bconst\b", "", ctype).strip()
        if ctype.endswith("*"):
            t = C.c_void_p
        elif ctype in _SCALARS:
            t = _SCALARS[ctype]
        else:
            assert ctype.endswith("_t"), (name, tag, field, ctype)
            t = ctypes_from_header(ctype[:-2])
        n = array_length(name, length)
        fields.append((field, t if n is None else t * n))
    return type(tag, (C.Structure,), {"_fields_": fields})


def same_ctype(a, b):
    """Two ctypes types are the same C type: the same scalar, arrays of the same length and element, structs of the same fields"""
    if issubclass(a, C.Structure) and issubclass(b, C.Structure):
        return len(a._fields_) == len(b._fields_) and all(na == nb and same_ctype(ta, tb) for (na, ta), (nb, tb) in zip(a._fields_, b._fields_))
    if issubclass(a, C.Array) and issubclass(b, C.Array):
        return a._length_ == b._length_ and same_ctype(a._type_, b._type_)
    return a is b


def layout(cls):
    """(sizeof, {field: offset}) of a ctypes Structure"""
    return C.sizeof(cls), {f[0]: getattr(cls, f[0]).offset for f in cls._fields_}


@functools.lru_cache(maxsize=None)
def compiler_layout(names):
    """{tag: (sizeof, {field: offset})} of every struct of the headers `names` (a tuple), from ONE C program that includes them all and
    prints sizeof and every offsetof, built with the system's C compiler; None where there is none."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        return None
    lines = ["#include <stdio.h>", "#include <stddef.h>"] + [f'#include "{n}"' for n in names] + ["int main(void) {"]
    for n in names:
        for tag, fields in read(n).structs.items():
            lines.append(f'  printf("{tag} . %zu\\n", sizeof({tag}_t));')
            lines += [f'  printf("{tag} {f} %zu\\n", offsetof({tag}_t, {f}));' for _, f, _ in fields]
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.run([cc, "-I", INCLUDE, src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {}
    for tag, field, value in (ln.split() for ln in out.splitlines()):
        size, offsets = got.setdefault(tag, [None, {}])
        if field == ".":
            got[tag][0] = int(value)
        else:
            offsets[field] = int(value)
    return {tag: (size, offsets) for tag, (size, offsets) in got.items()}
