"""The C ABI as text: include/zkhip.h, the declaration of record, and its hand-written mirrors include/zkhip.hpp and the `extern "C"` block of
rust-shim/zkhip_ffi.rs, read as declarations.  A helper module (no tests, no fixtures): tests/test_abi_mirrors.py checks every mirror against
the header through it, and the feature files compare their pinned tables with what it returns."""
import functools
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


def _strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _norm(decl):
    """one spelling per declaration: single spaces, every run of `*` against the name (`const void *const *d_columns`, `const char *`); an array
    extent stays as written"""
    decl, bracket, extent = " ".join(decl.split()).partition("[")
    decl = re.sub(r"(?<![(*])\*+", lambda m: " " + m.group(0), re.sub(r"\s*\*\s*", "*", decl))
    return (decl + bracket + extent).strip()


def _arguments(text, start):
    """the top-level comma-separated pieces of the bracket that opens just before text[start], and the index behind its closing bracket"""
    depth, i, pieces, piece = 1, start, [], start
    while depth:
        ch = text[i]
        depth += (ch in "([{") - (ch in ")]}")
        if depth == 0 or (ch == "," and depth == 1):
            pieces.append(text[piece:i])
            piece = i + 1
        i += 1
    return ([] if len(pieces) == 1 and not pieces[0].strip() else pieces), i


@functools.lru_cache(None)
def _declarations():
    text = _strip_comments(_read("include", "zkhip.h"))
    structs = {}
    for m in re.finditer(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = structs[m.group(2)] = []
        for decl in filter(None, (_norm(d) for d in m.group(1).split(";"))):
            one = r"\w+(?:\[[^\]]*\])*"                                                               # `zkhip_vm_operand a, b, c`, `uint64_t point[4]`
            ty, names = re.fullmatch(r"(.*?[\s*])(" + one + r"(?:\s*,\s*" + one + r")*)", decl).groups()
            for name, suffix in re.findall(r"(\w+)((?:\[[^\]]*\])*)", names):
                fields.append((ty.strip() + suffix, name))
    enums = {name: int(value) for body in re.findall(r"\benum\s*\{(.*?)\}", text, flags=re.S) for name, value in re.findall(r"(\w+)\s*=\s*(\d+)", body)}
    defines = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(ZKHIP_\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M):
        if re.fullmatch(r"\(?-?\d+u?\)?", value):
            defines[name] = int(value.strip("()u"))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)                                               # a macro's value is no return type
    text = re.sub(r"\{[^{}]*\}", "", text.replace('extern "C" {', ""))                                # nor is a struct's or an enum's body
    functions = {}
    for m in re.finditer(r"([\w\s*]+?)\b(zkhip_\w+)\s*\(", text):
        if m.group(1).split()[:1] == ["typedef"]:
            continue
        pieces, end = _arguments(text, m.end())
        assert text[end:].lstrip().startswith(";"), f"include/zkhip.h: {m.group(2)} is not a plain declaration"
        params = []
        for p in [] if [q.strip() for q in pieces] == ["void"] else pieces:
            p = _norm(p)
            ty, name, suffix = (re.fullmatch(r"(.*\(\*)(\w+)(\))(\[.*\])", p) or re.fullmatch(r"(.*?[\s*])(\w+)()((?:\[[^\]]*\])*)", p)).group(1, 2, 4)
            params.append((ty.strip() + (")" if ty.endswith("(*") else ""), name, suffix, p))
        assert m.group(2) not in functions, f"include/zkhip.h declares {m.group(2)} twice"
        functions[m.group(2)] = (_norm(m.group(1)), params)
    return functions, structs, defines, enums


def functions():
    """{name: (return type, [(type, parameter name, array suffix), ...])} for every function include/zkhip.h declares; `char (*names)[64]` is
    ("char (*)", "names", "[64]")"""
    return {name: (ret, [p[:3] for p in params]) for name, (ret, params) in _declarations()[0].items()}


def params(name):
    """the parameters of one function as the header spells them, whitespace normalised: ["const void *const *d_columns", "uint32_t n_columns", ...]"""
    assert name in _declarations()[0], f"include/zkhip.h does not declare {name}"
    return [p[3] for p in _declarations()[0][name][1]]


def structs():
    """{name: [(type, field), ...]} for every `typedef struct ... { ... } name;` with a body; an array field's type carries its extent (`uint64_t[4]`)"""
    return _declarations()[1]


def defines():
    """{name: value} of the numeric ZKHIP_* macros"""
    return _declarations()[2]


def enums():
    """{name: value} of the enumerators (ZKHIP_SRC_*, ZKHIP_OP_*)"""
    return _declarations()[3]


@functools.lru_cache(None)
def rust_functions():
    """{name: (return type or None, ["pname: type", ...])} of the `extern "C"` block of rust-shim/zkhip_ffi.rs"""
    block = re.search(r'^extern\s+"C"\s*\{(.*?)\n\}', _strip_comments(_read("rust-shim", "zkhip_ffi.rs")), flags=re.S | re.M)
    assert block, 'no extern "C" block in rust-shim/zkhip_ffi.rs'
    out = {}
    for name, args, ret in re.findall(r"\bfn\s+(\w+)\s*\((.*?)\)\s*(?:->\s*([^;]+?))?\s*;", block.group(1), flags=re.S):
        out[name] = (" ".join(ret.split()) or None, [" ".join(p.split()) for p in args.split(",") if p.strip()])
    return out


@functools.lru_cache(None)
def _hpp():
    return _strip_comments(_read("include", "zkhip.hpp"))


def hpp_call_arities(name):
    """the number of arguments of every call of `name` in include/zkhip.hpp, in file order"""
    return [len(_arguments(_hpp(), m.end())[0]) for m in re.finditer(r"\b" + name + r"\s*\(", _hpp())]


@functools.lru_cache(None)
def exported():
    """the names libzkhip.so defines in its dynamic symbol table"""
    from zksnap_circuits_halo2_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.split()}
