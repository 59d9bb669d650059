"""The ARX_* environment switches have one home and one inventory (no GPU, no library: a check of the text).

arachne_amd/csrc/switches.h is the only file of the product sources and of the host test double that reads the environment; every switch
is a field there (the double's own few are declared in tests/hostsim/sim.cpp through the same helpers).  DESIGN.md section 13 lists them
with accepted values, default, read time and kind.  These tests hold the three together, so that a switch cannot appear, vanish or be used
by a test or tool without the table saying what it is.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arachne_amd", "csrc")
SIM = os.path.join(ROOT, "tests", "hostsim", "sim.cpp")
NAME = r"ARX_[A-Z0-9_]+"


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _design_section(title):
    """the text of DESIGN.md's '### <title> ...' subsection, up to the next heading"""
    m = re.search(r"^### " + re.escape(title) + r"[^\n]*\n(.*?)(?=^#{1,3} |\Z)", _read(os.path.join(ROOT, "DESIGN.md")), re.S | re.M)
    assert m, "DESIGN.md has no subsection " + title
    return m.group(1)


def _table_names(title):
    rows = re.findall(r"^\| `(" + NAME + r")` \|", _design_section(title), re.M)
    assert len(rows) == len(set(rows)), "a switch has two rows in DESIGN.md " + title
    return set(rows)


def _listed_names(title):
    return set(re.findall(r"`(" + NAME + r")`", _design_section(title)))


def _quoted_names(path):
    return set(re.findall(r'"(' + NAME + r')"', _read(path)))


def test_only_switches_h_reads_the_environment():
    files = sorted(glob.glob(os.path.join(CSRC, "*"))) + [SIM]
    assert os.path.join(CSRC, "switches.h") in files
    hits = [os.path.relpath(p, ROOT) for p in files if os.path.basename(p) != "switches.h" and os.path.isfile(p) and "getenv(" in _read(p)]
    assert hits == [], "getenv( outside switches.h: %s" % hits


def test_design_table_is_the_set_switches_h_reads():
    read = _quoted_names(os.path.join(CSRC, "switches.h"))
    table = _table_names("13.1")
    assert read, "switches.h names no switch"
    assert read == table, "only in switches.h: %s; only in DESIGN.md 13.1: %s" % (sorted(read - table), sorted(table - read))
    sim, sim_table = _quoted_names(SIM), _table_names("13.2")
    assert sim == sim_table, "only in sim.cpp: %s; only in DESIGN.md 13.2: %s" % (sorted(sim - sim_table), sorted(sim_table - sim))
    assert not (table & sim_table)


def test_tests_and_tools_use_only_listed_switches():
    """Every ARX_* name a file under tests/ or tools/ mentions -- which covers every one it sets, however it spells the assignment -- is a
    run-time switch of the tables or a variable of the list of those read outside the library.  Names that are not environment variables
    at all are set aside first: the C ABI's constants (include/arachne_amd.h), preprocessor macros of the sources and the compile-time list."""
    known = _table_names("13.1") | _table_names("13.2") | _listed_names("13.4")
    not_env = set(re.findall(r"\b(" + NAME + r")\b", _read(os.path.join(ROOT, "include", "arachne_amd.h")))) | _listed_names("13.3")
    for p in glob.glob(os.path.join(CSRC, "*")) + [SIM]:
        not_env |= set(re.findall(r"^\s*#\s*(?:define|ifdef|ifndef)\s+(" + NAME + r")\b", _read(p), re.M))
    users = [p for pat in ("tests/*.py", "tests/golden/*.py", "tools/*") for p in glob.glob(os.path.join(ROOT, pat)) if os.path.isfile(p)]
    assert len(users) > 20
    unknown = {}
    for p in users:
        for n in set(re.findall(r"\b(" + NAME + r")\b", _read(p))) - known - not_env:
            unknown.setdefault(n, []).append(os.path.relpath(p, ROOT))
    assert unknown == {}, "ARX_* names used by tests or tools that DESIGN.md section 13 does not list: %s" % unknown
