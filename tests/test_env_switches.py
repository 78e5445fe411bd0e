"""Every GGML_MI355X_* run-time switch the sources read is listed in INTEGRATION.md's table (§6), and the table lists nothing else."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "llama.cpp-gfx906_amd" / "csrc"

# a switch is read by getenv or by one of csrc/env_switch.h's helpers; include/ggml-mi355x.h's GGML_MI355X_NAME, GGML_MI355X_MAX_DEVICES, ... are
# macros, never the string argument of such a call
READ = re.compile(r'\b(?:getenv|env_int|env_on|env_double|env_is_set)\s*\(\s*"(GGML_MI355X_[A-Z0-9_]+)"')
ROW = re.compile(r'^\|\s*`(GGML_MI355X_[A-Z0-9_]+)`\s*\|(.*)\|\s*$')


def switches_read():
    found = {}
    for path in sorted(CSRC.rglob("*")):
        if path.is_file() and path.suffix in (".h", ".hip", ".cpp"):
            for name in READ.findall(path.read_text()):
                found.setdefault(name, set()).add(path.name)
    return found


def table_rows():
    rows = {}
    for line in (ROOT / "INTEGRATION.md").read_text().splitlines():
        m = ROW.match(line)
        if m:
            assert m.group(1) not in rows, f"{m.group(1)} is listed twice"
            rows[m.group(1)] = [c.strip() for c in m.group(2).split("|")]
    return rows


def test_switch_table_lists_exactly_the_switches_the_sources_read():
    read, rows = switches_read(), table_rows()
    assert len(read) >= 30, "the scan found too few switches: has the call form changed?"
    assert set(read) - set(rows) == set(), "read in csrc/ but missing from INTEGRATION.md's table"
    assert set(rows) - set(read) == set(), "listed in INTEGRATION.md's table but read nowhere in csrc/"


def test_switch_table_names_the_file_that_reads_each_switch():
    read, rows = switches_read(), table_rows()
    for name, cells in rows.items():
        assert len(cells) == 3 and all(cells), (name, cells)
        assert cells[2].strip("`") in read.get(name, ()), (name, cells[2], read.get(name))


def test_switches_are_parsed_only_by_the_helper_header():
    for path in sorted(CSRC.glob("*")):
        if path.is_file() and path.name != "env_switch.h":
            assert 'getenv("GGML_MI355X_' not in path.read_text(), path.name
