"""Every MBFT_* environment variable the library reads has a row in
INTEGRATION.md's table, and every row names a variable the library reads."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minbft_amd", "csrc")

# an environment read: getenv or one of env.h's readers, first argument a literal
READ = re.compile(r'\b(?:getenv|env_[a-z0-9]+)\(\s*"(MBFT_[A-Z0-9_]+)"')


def read_by_library():
    names = set()
    for f in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, f), errors="replace") as fh:
            names.update(READ.findall(fh.read()))
    return names


def documented():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        text = fh.read()
    section = text[text.index("Environment knobs"):]
    names = set()
    rows = [l for l in section.splitlines() if l.startswith("| `MBFT_")]
    for row in rows:
        names.update(re.findall(r"`(MBFT_[A-Z0-9_]+)`", row.split("|")[1]))
    return names


def test_env_knobs_match_integration_table():
    code, doc = read_by_library(), documented()
    assert len(code) > 20 and len(doc) > 20  # the scan found the reads and the table
    assert code - doc == set(), "read by the library, no row in INTEGRATION.md"
    assert doc - code == set(), "a row in INTEGRATION.md, read by nothing"

