"""INTEGRATION.md, "Environment switches", lists exactly the VS_* variables the package reads: a removed switch leaves
the table with its code, a new one enters it with its default."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PY_READ = re.compile(r"""environ(?:\.get\(|\[)\s*["'](VS_[A-Z0-9_]+)["']""")
C_READ = re.compile(r"""(?:getenv|pw_env)\(\s*"(VS_[A-Z0-9_]+)\"""")


def _read_by_sources():
    names = set()
    for pattern, rx in (("vidsitu_amd/*.py", PY_READ), ("vidsitu_amd/csrc/*.hip", C_READ), ("vidsitu_amd/csrc/*.h", C_READ)):
        for path in glob.glob(os.path.join(ROOT, pattern)):
            with open(path) as f:
                names.update(rx.findall(f.read()))
    return names


def _documented():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    m = re.search(r"^## Environment switches\n(.*?)(?=^## |\Z)", text, re.M | re.S)
    assert m, "INTEGRATION.md has no section 'Environment switches'"
    rows = re.findall(r"^\| `(VS_[A-Z0-9_]+)` \| ([^|]+) \| ([^|]+) \|$", m.group(1), re.M)
    names = [r[0] for r in rows]
    assert len(names) == len(set(names)), "a switch is listed twice"
    assert all(d.strip() and t.strip() for _, d, t in rows), "every switch has a default and one line"
    return set(names)


def test_documented_switches_are_the_ones_the_sources_read():
    read, listed = _read_by_sources(), _documented()
    assert len(read) > 40, "the source scan found too few switches to be right"
    assert read - listed == set(), f"read by the sources, missing from INTEGRATION.md: {sorted(read - listed)}"
    assert listed - read == set(), f"listed in INTEGRATION.md, read by no source: {sorted(listed - read)}"
