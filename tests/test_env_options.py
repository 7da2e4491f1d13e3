"""The environment variables of the project, read from the tree: what the library and the Python package read, what INTEGRATION.md's
environment table documents, and what the tests and tools set are one list.  A variable that is read but not documented, documented but
not read, or set by a test or advertised by a tool and read by nothing fails here.  CPU only: no library is loaded."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = r"ZKHIP_[A-Z0-9_]*[A-Z0-9]"


def text(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def files(*patterns):
    return sorted(p for pat in patterns for p in glob.glob(os.path.join(ROOT, pat), recursive=True) if os.path.isfile(p))


def python_lookups(src):
    """names a Python source looks up in the environment: os.environ.get("X"...), os.environ["X"] as a value, os.getenv("X")"""
    names = set(re.findall(r"os\.environ\.get\(\s*[\"'](%s)[\"']" % NAME, src)) | set(re.findall(r"os\.getenv\(\s*[\"'](%s)[\"']" % NAME, src))
    names |= set(re.findall(r"os\.environ\[[\"'](%s)[\"']\](?!\s*=[^=])" % NAME, src))
    return names


def library_reads():
    return {n for p in files("zksnap_circuits_halo2_amd/csrc/*") for n in re.findall(r"getenv\(\s*\"(%s)\"\s*\)" % NAME, text(p))}


def package_reads():
    return {n for p in files("zksnap_circuits_halo2_amd/*.py") for n in python_lookups(text(p))}


def table_rows():
    """{name: the row's first cell} of the table under INTEGRATION.md's `| variable | effect |` header"""
    lines = text(os.path.join(ROOT, "INTEGRATION.md")).split("\n")
    start = lines.index("| variable | effect |") + 2
    rows = {}
    for line in lines[start:]:
        if not line.startswith("|"):
            break
        cell = line.split("|")[1].replace("`", "")
        for n in re.findall(NAME, cell):
            rows[n] = cell
    return rows


def abi_constants():
    """ZKHIP_* names that are constants of the C ABI (error codes, limits, enumerators), not environment variables"""
    h = text(os.path.join(ROOT, "include", "zkhip.h"))
    return set(re.findall(r"#define\s+(%s)\b" % NAME, h)) | set(re.findall(r"^\s*(%s)\s*(?:=[^=]|,)" % NAME, h, flags=re.M))


def test_every_variable_read_is_documented():
    read, rows = library_reads() | package_reads(), table_rows()
    assert len(library_reads()) >= 10 and "ZKHIP_LIB_PATH" in package_reads() and len(rows) >= 10      # the scans found their subjects
    assert sorted(read - set(rows)) == []


def test_every_documented_variable_is_read():
    read = library_reads() | package_reads()
    elsewhere = ("bench.py only", "rust-shim only")      # read by bench.py / by the Rust shim of INTEGRATION.md, which is not in this tree
    stale = sorted(n for n, cell in table_rows().items() if n not in read and not any(m in cell for m in elsewhere))
    assert stale == []


def test_every_variable_set_by_tests_and_tools_is_read():
    read = library_reads() | package_reads() | python_lookups(text(os.path.join(ROOT, "bench.py")))
    constants = abi_constants()
    used = {}
    # tests: a name put into an environment -- os.environ["X"] = ..., env["X"] = ..., setenv("X", ...), or a keyword of dict(os.environ, X=...)
    for p in files("tests/**/*.py"):
        if os.path.samefile(p, __file__):
            continue
        src = text(p)
        for n in (re.findall(r"\[[\"'](%s)[\"']\]\s*=[^=]" % NAME, src) + re.findall(r"setenv\(\s*[\"'](%s)[\"']" % NAME, src) +
                  re.findall(r"setdefault\(\s*[\"'](%s)[\"']" % NAME, src) + re.findall(r"\b(%s)\s*=[^=]" % NAME, src)):
            used.setdefault(n, os.path.relpath(p, ROOT))
    # tools: their usage texts advertise variables as well as set them, so every name a tool mentions counts
    for p in files("tools/**/*"):
        for n in re.findall(NAME, text(p)):
            used.setdefault(n, os.path.relpath(p, ROOT))
    assert "ZKHIP_VM_JIT" in used and "ZKHIP_TEST_DUPLICATE_DEVICES" in used      # the scans found their subjects
    unread = sorted((n, p) for n, p in used.items() if n not in read and n not in constants)
    assert unread == []
