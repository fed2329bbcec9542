"""The PROQA_* environment switches: the README table lists exactly what the sources read, no script sets a variable that
nothing reads, and the switches of retired experiments stay out of the library."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = r"PROQA_[A-Z0-9_]+"
# switches removed together with the experiments they selected
RETIRED = {
    "PROQA_FILTER_QW", "PROQA_FILTER_FLAGS", "PROQA_COMPACT_FLAG128", "PROQA_I8_DEEP_RING", "PROQA_I8_ROW_SPLIT",
    "PROQA_MERGE_NOM_CAP", "PROQA_MERGE_NOM_WIDE", "PROQA_EQUAL_GROWTH", "PROQA_GROWTH_LIST", "PROQA_CAND_BUDGET",
    "PROQA_GEMM_DBG", "PROQA_GEMM_EPI_SCALAR", "PROQA_FILTER_VARIANT", "PROQA_ENCODER_GRAPH", "PROQA_LOADER_PIECE_MB",
}


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _files(pattern):
    return sorted(p for p in glob.glob(os.path.join(ROOT, pattern)) if os.path.isfile(p))


def _library_reads():
    """Names handed to getenv / env_int in the library (debug_flag is mips_index.cpp's getenv(name) != nullptr)."""
    names = set()
    for path in _files("proqa_amd/csrc/*"):
        if path.endswith((".cpp", ".hip", ".h", ".inc")):
            names |= set(re.findall(r'\b(?:getenv|env_int|debug_flag)\(\s*"(%s)"' % NAME, _read(path)))
    return names


def _python_reads(paths):
    names = set()
    for path in paths:
        names |= set(re.findall(r'(?:environ\.get\(|environ\[|getenv\()\s*["\'](%s)["\']' % NAME, _read(path)))
    return names


def _readme_table():
    """{section title: names} of the 'Environment switches' table: a row whose first cell is bold opens a section."""
    text = _read(os.path.join(ROOT, "README.md"))
    body = text.split("### Environment switches", 1)[1].split("\n#", 1)[0]
    sections, cur = {}, None
    for line in body.splitlines():
        if not line.startswith("|"):
            continue
        first = line.split("|")[1].strip()
        if first.startswith("**"):
            cur = first
            sections[cur] = set()
        elif cur is not None:
            m = re.fullmatch(r"`(%s)`" % NAME, first)
            assert m, f"switch table row without a variable name: {line}"
            assert m.group(1) not in sections[cur], f"{m.group(1)} is listed twice"
            sections[cur].add(m.group(1))
    return sections


def test_readme_table_lists_exactly_the_switches_the_sources_read():
    sections = _readme_table()
    assert len(sections) == 2, sorted(sections)
    (lib_title, lib_names), (py_title, py_names) = sections.items()
    assert "Library" in lib_title and "Python" in py_title
    assert lib_names == _library_reads()
    assert py_names == _python_reads(_files("proqa_amd/*.py"))


def test_no_script_sets_a_variable_that_nothing_reads():
    # (a script that reads a variable of its own from the environment counts as well: somebody is meant to set it)
    read = _library_reads() | _python_reads(_files("proqa_amd/*.py") + _files("*.py"))
    stale = {}
    for path in _files("scripts/*") + _files("scripts/native/*"):
        text = _read(path)
        # NAME=value in a shell line or a dict(os.environ, NAME=...) call (not ==, not -DNAME=), env["NAME"] = ..., export NAME
        sets = set(re.findall(r"(?<![-\w])(%s)=(?!=)" % NAME, text))
        sets |= set(re.findall(r'\[["\'](%s)["\']\]\s*=(?!=)' % NAME, text))
        sets |= set(re.findall(r"\bexport\s+(%s)\b" % NAME, text))
        sets |= _python_reads([path])
        if sets - read:
            stale[os.path.relpath(path, ROOT)] = sorted(sets - read)
    assert not stale, f"scripts set variables that nothing reads: {stale}"


def test_retired_switches_are_gone_from_the_library():
    found = {}
    for path in _files("proqa_amd/csrc/*"):
        if path.endswith(".so") or path.endswith(".o"):
            continue
        hit = RETIRED & set(re.findall(NAME, _read(path)))
        if hit:
            found[os.path.relpath(path, ROOT)] = sorted(hit)
    assert not found, found
    assert not RETIRED & (_library_reads() | _python_reads(_files("proqa_amd/*.py")))
