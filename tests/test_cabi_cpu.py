"""The C boundary, checked declaration by declaration: include/kai0hip.h against kai0_amd/_lib.py's prototype table and struct mirrors.

No GPU and no library: the header is parsed as text.  The parser refuses what it does not understand (an unknown statement, an unknown
type), so a declaration cannot drop out silently; what it found is additionally held against a plain count of `kai0_name(` in the
header.  ctypes checks nothing of this by itself: a `c_int` where the header says `int64_t` truncates a stride without a word."""

import ctypes as C
import os
import re

import pytest

from kai0_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kai0hip.h")
SCALARS = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "float": "f32", "double": "f64", "uint32_t": "u32"}
CTYPES_CODES = {"i": "i32", "l": "i64", "q": "i64", "f": "f32", "d": "f64", "I": "u32", "P": "ptr", "z": "ptr"}


def _statements(text):
    """The header's top-level statements (text up to a `;` outside braces), comments and preprocessor lines removed."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    head, sep, text = text.partition('extern "C" {')
    assert sep and not head.strip(), head
    text, sep, tail = text.rpartition("}")
    assert sep and not tail.strip(), tail
    out, depth, cur = [], 0, []
    for ch in text:
        depth += (ch == "{") - (ch == "}")
        assert depth >= 0
        if ch == ";" and depth == 0:
            out.append(" ".join("".join(cur).split()))
            cur = []
        else:
            cur.append(ch)
    assert depth == 0 and not "".join(cur).strip(), "".join(cur)
    return out, text


def _kind(ctype, aliases):
    """'ptr' / 'i32' / ... of a C type as written (`const float*`, `int64_t`, `kai0_stream_t`), or the name of a known struct."""
    if "*" in ctype:
        return "ptr"
    words = [w for w in ctype.split() if w != "const"]
    assert len(words) == 1, ctype
    (word,) = words
    if word in aliases:
        return aliases[word]
    assert word in SCALARS, f"unknown type {ctype!r}"
    return SCALARS[word]


def _fields(body, aliases):
    """[(name, kind)] of a struct body; kind is (element kind, length) for an array, a nested field list for an anonymous struct."""
    out, depth, cur, decls = [], 0, [], []
    for ch in body:
        depth += (ch == "{") - (ch == "}")
        if ch == ";" and depth == 0:
            decls.append(" ".join("".join(cur).split()))
            cur = []
        else:
            cur.append(ch)
    assert not "".join(cur).strip(), "".join(cur)
    for decl in decls:
        m = re.fullmatch(r"struct \{(.*)\} (\w+)\[(\d+)\]", decl)
        if m:  # `struct { ... } seg[3]`
            out.append((m.group(2), (_fields(m.group(1), aliases), int(m.group(3)))))
            continue
        first, *more = [d.strip() for d in decl.split(",")]
        m = re.fullmatch(r"(.*?[\s*])(\w+)(\[(\d+)\])?", first)
        assert m and all(re.fullmatch(r"\w+", x) for x in more), decl
        kind = _kind(m.group(1).strip(), aliases)
        assert not (more and (kind == "ptr" or m.group(3))), decl  # `T *a, *b` and `T a[2], b` are not written in this header
        out.append((m.group(2), (kind, int(m.group(4))) if m.group(3) else kind))
        out += [(name, kind) for name in more]
    return out


def parse_header():
    """-> (functions {name: (return kind, [argument kinds])}, structs {name: [(field, kind)]}, the stripped text)."""
    statements, text = _statements(open(HEADER).read())
    aliases, functions, structs = {}, {}, {}
    for st in statements:
        m = re.fullmatch(r"typedef struct (\w+) \{(.*)\} (\w+)", st)
        if m:
            assert m.group(1) == m.group(3), st
            structs[m.group(3)] = _fields(m.group(2), aliases)
            aliases[m.group(3)] = m.group(3)  # by value: the struct's name stands for its kind
            continue
        m = re.fullmatch(r"typedef (.*?[\s*])(\w+)", st)
        if m:
            aliases[m.group(2)] = _kind(m.group(1).strip(), aliases)
            continue
        m = re.fullmatch(r"(.*?[\s*])(kai0_\w+)\((.*)\)", st)
        assert m, f"not a declaration this parser knows: {st!r}"
        args = [] if m.group(3).strip() == "void" else [a.strip() for a in m.group(3).split(",")]
        kinds = []
        for a in args:
            am = re.fullmatch(r"(.*?[\s*])(\w+)", a)
            assert am, a
            kinds.append(_kind(am.group(1).strip(), aliases))
        assert m.group(2) not in functions, m.group(2)
        functions[m.group(2)] = (_kind(m.group(1).strip(), aliases), kinds)
    return functions, structs, text


def ctypes_kind(t):
    if t is None:
        return "void"
    if isinstance(t, type) and issubclass(t, C._Pointer):
        return "ptr"
    if isinstance(t, type) and issubclass(t, C.Array):
        return (ctypes_kind(t._type_), t._length_)
    if isinstance(t, type) and issubclass(t, C.Structure):
        names = [n for n, m in _lib.MIRRORS.items() if m is t]
        return names[0] if names else mirror_fields(t)  # a named struct of the header, or an anonymous nested one
    kind = CTYPES_CODES[t._type_]
    assert C.sizeof(t) == {"ptr": 8, "i32": 4, "i64": 8, "f32": 4, "f64": 8, "u32": 4}[kind], t
    return kind


def mirror_fields(mirror):
    return [(name, ctypes_kind(t)) for name, t in mirror._fields_]


def prototype_mismatches(functions, protos, restype_of):
    """Names whose argument kinds or return kind differ between the header and the table (names in both only)."""
    bad = []
    for name in sorted(set(functions) & set(protos)):
        got = (ctypes_kind(restype_of(name)), [ctypes_kind(t) for t in protos[name]])
        if got != functions[name]:
            bad.append(f"{name}: header {functions[name]} != table {got}")
    return bad


@pytest.fixture(scope="module")
def header():
    return parse_header()


def test_every_declaration_is_found(header):
    functions, structs, text = header
    assert len(functions) == len(re.findall(r"\bkai0_\w+\s*\(", text))  # the parser skipped nothing that looks like a declaration
    assert len(structs) == len(re.findall(r"\btypedef\s+struct\b", text))
    assert set(functions) == set(_lib.EXPORTED_SYMBOLS), set(functions) ^ set(_lib.EXPORTED_SYMBOLS)
    assert len(_lib.EXPORTED_SYMBOLS) == len(set(_lib.EXPORTED_SYMBOLS)) and tuple(_lib._PROTOS) == _lib.EXPORTED_SYMBOLS


def test_prototypes_match_the_header(header):
    functions = header[0]
    assert prototype_mismatches(functions, _lib._PROTOS, _lib.restype_of) == []


def test_a_missing_restype_is_noticed(header):
    """The functions that do not return int: with the restype taken out of the table (ctypes' default, int) each one is reported."""
    functions = header[0]
    non_int = sorted(n for n, (ret, _) in functions.items() if ret != "i32")
    assert len(non_int) == 7 and "kai0_gemm_f32_workspace_bytes" in non_int and "kai0_last_error" in non_int
    for name in non_int:
        bad = prototype_mismatches(functions, _lib._PROTOS, lambda n: C.c_int if n == name else _lib.restype_of(n))
        assert len(bad) == 1 and bad[0].startswith(name + ":"), bad
    # ... and a narrowed argument likewise: kai0_rope_copy's first stride as c_int
    protos = dict(_lib._PROTOS)
    i = functions["kai0_rope_copy"][1].index("i64")
    protos["kai0_rope_copy"] = [C.c_int if j == i else t for j, t in enumerate(protos["kai0_rope_copy"])]
    bad = prototype_mismatches(functions, protos, _lib.restype_of)
    assert len(bad) == 1 and bad[0].startswith("kai0_rope_copy:"), bad


def test_struct_mirrors_match_the_header(header):
    structs = dict(header[1])
    # the engine builds kai0_ck_item as an int64 [n, 2] tensor (kai0_amd/infer.py): two 8-byte fields, no mirror
    assert structs.pop("kai0_ck_item") == [("ptr", "ptr"), ("nbytes", "i64")]
    assert set(structs) == set(_lib.MIRRORS), set(structs) ^ set(_lib.MIRRORS)
    for name, fields in structs.items():
        assert mirror_fields(_lib.MIRRORS[name]) == fields, name
    nested = dict(structs["kai0_gemm_desc"])["seg"]
    assert nested == (mirror_fields(_lib.GemmSeg), 3) and dict(structs["kai0_skinny_desc"])["seg"] == ("kai0_skinny_seg", 3)
    # every kai0_X_size() has the struct it measures (what load() looks up)
    for fn in _lib._PROTOS:
        if fn.endswith("_size"):
            assert fn[:-5] in _lib.MIRRORS or fn[:-5] + "_t" in _lib.MIRRORS, fn
