"""The native C API (the extern "C" dct_* launchers of csrc/) has one checked declaration per entry point.

Every launcher takes void* streams and raw pointers, so a prototype that disagrees with its definition
compiles, links and runs with shifted arguments - unless the compiler sees both in one translation unit.
Text only (no build, no GPU, no import of the extension): the sources are read with comments and string
literals removed, and every `<type> dct_name(...)` is classified by what follows its parameter list - `{` a
definition, `;` a declaration.

  (a) every dct_* function defined in a .hip / .cpp is declared in exactly one .h;
  (b) the defining file reaches that header through its #include "..." chain;
  (c) no .hip / .cpp declares a dct_* function without a body (a private prototype nothing checks)."""
import glob
import os
import re

import pytest

(CSRC,) = glob.glob(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "*", "csrc"))

_NOT_A_TYPE = {"return", "else", "case", "goto", "throw", "new", "delete", "co_return", "sizeof", "typedef", "using"}
_TYPE = re.compile(r"(?:extern_C\s+)?[A-Za-z_][\w:]*(?:\s+[A-Za-z_][\w:]*)*[\s*]*\Z")
_NAME = re.compile(r"\b(dct_\w+)\s*\(")
_STOP = re.compile(r"[;{}()=,!?|<>+\-/#\[\]]")


def _strip(text):
    """Comments, string and character literals out (newlines kept); extern "C" kept as one word."""
    text = re.sub(r'extern\s+"C"', "extern_C", text)
    pat = re.compile(r'//[^\n]*|/\*.*?\*/|"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'', re.S)
    return pat.sub(lambda m: "\n" * m.group(0).count("\n") if m.group(0)[0] == "/" else '""', text)


def _close(text, i):
    """Index just past the parenthesis that closes the one at text[i]."""
    depth = 0
    for j in range(i, len(text)):
        depth += (text[j] == "(") - (text[j] == ")")
        if depth == 0:
            return j + 1
    raise ValueError("unbalanced parentheses")


def _scan(text):
    """[(name, "def" | "decl", is_static, line)] of the dct_* functions a source text defines or declares."""
    out = []
    text = _strip(text)
    for m in _NAME.finditer(text):
        start = m.start(1)
        stops = [s.end() for s in _STOP.finditer(text, max(0, start - 200), start)]
        prefix = text[(stops[-1] if stops else max(0, start - 200)):start]
        words = prefix.split()
        if not words or not _TYPE.match(prefix.strip() + " ") or _NOT_A_TYPE & set(re.findall(r"\w+", prefix)):
            continue  # a call, not a declarator
        after = text[_close(text, m.end() - 1):].lstrip()
        kind = {"{": "def", ";": "decl"}.get(after[:1])
        if kind:
            out.append((m.group(1), kind, "static" in words, text.count("\n", 0, start) + 1))
    return out


def _files(*suffixes):
    return sorted(f for f in os.listdir(CSRC) if f.endswith(suffixes))


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _reach(name, seen=None):
    """The csrc files `name` includes, directly or through other csrc files."""
    seen = set() if seen is None else seen
    for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', _read(name), re.M):
        if inc not in seen and os.path.exists(os.path.join(CSRC, inc)):
            seen.add(inc)
            _reach(inc, seen)
    return seen


@pytest.fixture(scope="module")
def api():
    scans = {f: _scan(_read(f)) for f in _files(".hip", ".cpp", ".h")}
    declared = {}  # name -> headers with a body-less declaration of it
    for f in _files(".h"):
        for name, kind, _, _ in scans[f]:
            if kind == "decl":
                declared.setdefault(name, []).append(f)
    defined = [(f, name) for f in _files(".hip", ".cpp") for name, kind, static, _ in scans[f]
               if kind == "def" and not static]
    return scans, declared, defined


def test_scanner_tells_definitions_declarations_and_calls():
    text = '''extern "C" {
    // int dct_in_comment(int a);
    int dct_decl(const float* p, void (*cb)(int), void* stream);
    int64_t dct_def(int64_t n) { return dct_call(n) + (n ? dct_call2(n) : 0); }
    static int dct_local(int a) { if (a) dct_stmt(a); return 0; }
    }
    const char* s = "int dct_in_string(int);";'''
    assert _scan(text) == [("dct_decl", "decl", False, 3), ("dct_def", "def", False, 4), ("dct_local", "def", True, 5)]


def test_sources_are_found(api):
    _, declared, defined = api
    assert len(defined) > 50 and len(declared) > 50  # an empty scan would pass the checks below


def test_every_entry_point_is_declared_in_exactly_one_header(api):
    _, declared, defined = api
    bad = [f"{name} ({f}): declared in {declared.get(name, []) or 'no header'}"
           for f, name in defined if len(declared.get(name, [])) != 1]
    assert not bad, "\n".join(bad)


def test_every_definer_includes_its_declaration(api):
    _, declared, defined = api
    bad = [f"{name}: {f} does not include {declared[name][0]}"
           for f, name in defined if len(declared.get(name, [])) == 1 and declared[name][0] not in _reach(f)]
    assert not bad, "\n".join(bad)


def test_no_private_prototypes_in_translation_units(api):
    scans, _, _ = api
    bad = [f"{f}:{line}: {name}" for f in _files(".hip", ".cpp") for name, kind, _, line in scans[f] if kind == "decl"]
    assert not bad, "\n".join(bad)
