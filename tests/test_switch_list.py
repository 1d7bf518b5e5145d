"""INTEGRATION.md, "Environment switches", lists exactly the VS_* variables the package reads, with the defaults the code
has: the package's table (vidsitu_amd/switches.py), the library's (csrc/switches.h, asked through vs_switch_value of
the built library) and the document are held to each other, nothing reads the environment beside the two tables, and
the tools set no switch that nobody reads.  No GPU call anywhere in here."""
import glob
import json
import os
import re
import subprocess
import sys

import pytest

from vidsitu_amd import switches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBRARY = switches.library_table()  # parsed from the X(...) lines of csrc/switches.h: name -> (C type, default)

# one documented non-default value per library switch (INTEGRATION.md's "Meaning" column; sizes: another valid size)
OVERRIDES = {
    "VS_BC32_TPW": "6", "VS_BN_FIN2": "0", "VS_BN_NBMAX": "2", "VS_BN_TARGET": "1024", "VS_CONV_DEEP": "2",
    "VS_CONV_HALO": "0", "VS_CONV_KORDER_MIN": "3", "VS_CONV_PW": "2", "VS_CONV_SPLITK_IL": "1",
    "VS_CONV_SPLITK_IL_NK": "16", "VS_CONV_SPLITK_IL_TILES": "112", "VS_DIRECT_BNB": "1", "VS_DIRECT_TB": "4",
    "VS_DIRECT_TPW_BLOCKS": "512", "VS_HALO_CONFLICT_WEIGHT": "0.7", "VS_LN_BWD_FUSED": "0", "VS_PW_BN": "64",
    "VS_PW_DBG": "5", "VS_PW_EDBG": "2", "VS_PW_NSLOT": "7", "VS_PW_OCC": "1", "VS_STEM_PAIR": "2", "VS_WGG_JOBS": "1",
    "VS_WGG_SLOTS": "192", "VS_WGRAD_DBG": "3", "VS_WGRAD_DEEP": "0", "VS_WGRAD_DEEP_MINP": "10000",
    "VS_WGRAD_DEEP_STAG": "0", "VS_WGRAD_S1_TILES": "96", "VS_WGRAD_SLOTS": "768", "VS_WGRAD_SLOTS_SMALL": "2048",
    "VS_WGRAD_XCD": "2", "VS_WHATIF_LINEAR_DW": "1", "VS_WHATIF_OK": "1",
}

# the child loads the library and asks for every name on its command line; null = the library refused the name
CHILD = """
import ctypes, json, sys
from vidsitu_amd import _lib
lib, out = _lib.load(), {}
for name in sys.argv[1:]:
    v = ctypes.c_double(-12345.0)
    rc = lib.vs_switch_value(name.encode(), ctypes.byref(v))
    out[name] = v.value if rc == 0 else None
assert lib.vs_switch_value(b"VS_CONV_DEEP", None) == -1 and lib.vs_switch_value(None, ctypes.byref(v)) == -1
assert lib.vs_launch_count() == 0
print("ANSWERS " + json.dumps(out))
"""


def _documented():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    m = re.search(r"^## Environment switches\n(.*?)(?=^## |\Z)", text, re.M | re.S)
    assert m, "INTEGRATION.md has no section 'Environment switches'"
    rows = re.findall(r"^\| `(VS_[A-Z0-9_]+)` \| ([^|]+) \| ([^|]+) \|$", m.group(1), re.M)
    names = [r[0] for r in rows]
    assert len(names) == len(set(names)), "a switch is listed twice"
    assert all(d.strip() and t.strip() for _, d, t in rows), "every switch has a default and one line"
    return {n: (d.strip(), t.strip()) for n, d, t in rows}


def _number(default):
    """A library default as the number vs_switch_value answers; "unset" (VS_WHATIF_OK) is the library's 0."""
    return 0.0 if default == "unset" else float(default)


def _ask_library(extra_env):
    """{name: value or None} for every library switch and one unknown name, from a fresh process whose environment
    holds no VS_* variable but `extra_env`."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("VS_")}
    env.update(extra_env)
    r = subprocess.run([sys.executable, "-c", CHILD, *sorted(LIBRARY), "VS_NO_SUCH_SWITCH"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(re.search(r"^ANSWERS (.*)$", r.stdout, re.M).group(1))


def _sources(*patterns):
    for pattern in patterns:
        for path in sorted(glob.glob(os.path.join(ROOT, pattern), recursive=True)):
            with open(path) as f:
                yield os.path.relpath(path, ROOT), f.read()


def test_documented_switches_are_the_two_tables():
    listed = set(_documented())
    tables = set(switches.SWITCHES) | set(LIBRARY)
    assert len(tables) > 40, "the tables hold too few switches to be right"
    assert tables - listed == set(), f"in a table, missing from INTEGRATION.md: {sorted(tables - listed)}"
    assert listed - tables == set(), f"listed in INTEGRATION.md, in no table: {sorted(listed - tables)}"
    assert len(LIBRARY) > 30 and all(t in ("int", "long long", "double") for t, _ in LIBRARY.values())
    with open(os.path.join(ROOT, "vidsitu_amd", "csrc", "switches.h")) as f:
        assert len(re.findall(r"^\s*X\(", f.read(), re.M)) == len(LIBRARY), "an X(...) line the parser does not read"
    assert set(OVERRIDES) == set(LIBRARY)


def test_nothing_reads_the_environment_beside_the_tables():
    for path, text in _sources("vidsitu_amd/csrc/*.hip", "vidsitu_amd/csrc/*.h", "include/*.h"):
        if path != os.path.join("vidsitu_amd", "csrc", "switches.h"):
            assert "getenv" not in text, f"{path} reads the environment itself"
    stray = re.compile(r"""environ(?:\.get\(|\.pop\(|\.setdefault\(|\[)\s*["']VS_""")
    for path, text in _sources("vidsitu_amd/*.py"):
        if path != os.path.join("vidsitu_amd", "switches.py"):
            assert not stray.search(text), f"{path} reads a VS_* variable itself"


def test_library_defaults_are_the_documented_ones():
    doc, got = _documented(), _ask_library({})
    assert got.pop("VS_NO_SUCH_SWITCH") is None
    for name, (_, in_header) in LIBRARY.items():
        assert got[name] is not None, f"vs_switch_value refuses {name}"
        assert got[name] == _number(doc[name][0]), f"{name}: the library says {got[name]}, INTEGRATION.md {doc[name][0]}"
        assert float(in_header) == _number(doc[name][0]), name


def test_library_overrides_come_back_as_set():
    doc, got = _documented(), _ask_library(OVERRIDES)
    assert got.pop("VS_NO_SUCH_SWITCH") is None
    for name, text in OVERRIDES.items():
        assert float(text) != _number(doc[name][0]), f"{name}: the override is the default"
        assert got[name] == float(text), f"{name}={text}: the library says {got[name]}"
    assert float(OVERRIDES["VS_HALO_CONFLICT_WEIGHT"]) % 1 != 0


def test_package_defaults_are_the_documented_ones():
    doc = _documented()
    for name, sw in switches.SWITCHES.items():
        default, meaning = doc[name]
        assert sw.default == default, f"{name}: the table says {sw.default}, INTEGRATION.md {default}"
        assert sw.meaning == meaning, f"{name}: the table's line differs from INTEGRATION.md's"
        if default == "unset":
            assert switches.read(name, env={}) is None
        else:
            got = switches.read(name, env={})
            assert got is not None and got == switches.read(name, env={name: default}) and type(got) is not str
    on, off = switches.read("VS_DUAL_STREAM", env={}), switches.read("VS_RESIDUAL_FP32", env={})
    assert on is True and off is False and switches.read("VS_WGRAD_GROUP_SPAN", env={}) == 3
    assert switches.read("VS_BN_TWO_LEVEL", env={}) == 512 and switches.read("VS_WGRAD_GROUP_MINC", env={}) == 128
    assert switches.read("VS_ADAM_OVERLAP", env={}) == 0 and switches.read("VS_WHATIF", env={}) == 0


# kind -> (a switch of that kind, what the sites of that kind computed before there was a table)
OLD_RULES = {
    "on": ("VS_CONV_PAIR", lambda e: e.get("VS_CONV_PAIR", "1") != "0"),
    "off": ("VS_EVAL_SPLIT_WEIGHTS", lambda e: e.get("VS_EVAL_SPLIT_WEIGHTS", "0") == "1"),
    "adam": ("VS_ADAM_OVERLAP", lambda e: (e.get("VS_ADAM_OVERLAP", "0") not in ("0", ""), e.get("VS_ADAM_OVERLAP") == "2")),
    "fill": ("VS_GRAD_FILL", lambda e: ({"0": False, "1": True, "learn": "learn"}[e.get("VS_GRAD_FILL", "")]
                                        if e.get("VS_GRAD_FILL", "") in ("0", "1", "learn") else None)),
    "text": ("VS_LIB_PATH", lambda e: e.get("VS_LIB_PATH")),
}
STRINGS = [None, "", "0", "1", "2", "3", "-1", "01", " 1", "on", "true", "learn", "/tmp/lib.so"]


@pytest.mark.parametrize("kind", sorted(OLD_RULES))
def test_each_kind_keeps_its_sites_rule_for_every_string(kind):
    name, old = OLD_RULES[kind]
    assert switches.SWITCHES[name].kind == kind
    for s in STRINGS:
        env = {} if s is None else {name: s}
        got = switches.read(name, env=env)
        if kind == "adam":  # train_step.py asks twice: `!= 0` where it read `not in ("0", "")`, `== 2` where `== "2"`
            got = (got != 0, got == 2)
        assert got == old(env) and type(got) is type(old(env)), f"{name}={s!r}: {got!r}, was {old(env)!r}"


def test_integer_kind_is_int_of_the_string():
    for s in ("0", "1", "2", "7", "-3", " 12 "):
        assert switches.read("VS_WGRAD_GROUP_SPAN", env={"VS_WGRAD_GROUP_SPAN": s}) == int(s)
    for s in ("", "x", "1.5"):
        with pytest.raises(ValueError):
            switches.read("VS_BN_TWO_LEVEL", env={"VS_BN_TWO_LEVEL": s})
    assert {n for n, sw in switches.SWITCHES.items() if sw.kind == "int"} == {
        "VS_WGRAD_GROUP_SPAN", "VS_WGRAD_GROUP_MINC", "VS_BN_TWO_LEVEL", "VS_WHATIF"}
    assert {sw.kind for sw in switches.SWITCHES.values()} == set(OLD_RULES) | {"int"}


def test_whatif_is_refused_without_its_guard():
    with pytest.raises(RuntimeError, match="VS_WHATIF_OK=1"):
        switches.read("VS_WHATIF", env={"VS_WHATIF": "4"})
    with pytest.raises(RuntimeError):
        switches.read("VS_WHATIF", env={"VS_WHATIF": "4", "VS_WHATIF_OK": "2"})
    assert switches.read("VS_WHATIF", env={"VS_WHATIF": "4", "VS_WHATIF_OK": "1"}) == 4
    assert switches.read("VS_WHATIF", env={"VS_WHATIF": "0"}) == 0
    # ... and importing ops is what asks
    env = {k: v for k, v in os.environ.items() if not k.startswith("VS_")}
    r = subprocess.run([sys.executable, "-c", "import vidsitu_amd.ops"], cwd=ROOT, env=dict(env, VS_WHATIF="4"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "RuntimeError: VS_WHATIF skips kernel launches" in r.stderr, r.stderr[-2000:]


def test_tools_set_only_switches_somebody_reads():
    known = set(switches.SWITCHES) | set(LIBRARY)
    read = re.compile(r"""(?:environ\.get\(\s*|getenv\(\s*|environ\[\s*)["'](VS_[A-Z0-9_]+)["']\]?(?!\]?\s*=[^=])"""
                      r"""|\$\{?(VS_[A-Z0-9_]+)""")
    for _, text in _sources("bench.py", "tests/*.py", "tools/**/*.py", "tools/**/*.sh"):
        known.update(a or b for a, b in read.findall(text))
    sets = set()
    for path, text in _sources("tools/**/*.sh"):
        sets.update((m.group(2), path) for m in re.finditer(r"(?<![A-Za-z0-9_])(-D)?(VS_[A-Z0-9_]+)=", text)
                    if not m.group(1))  # -DVS_YST=1: a compile flag (tools/build_variant_lib.sh)
    for path, text in _sources("tools/**/*.py"):
        sets.update((n, path) for n in re.findall(r"""environ\[["'](VS_[A-Z0-9_]+)["']\]\s*=[^=]""", text))
    assert len({n for n, _ in sets}) > 30, "the scan of tools/ found too few assignments to be right"
    dead = sorted((n, p) for n, p in sets if n not in known)
    assert dead == [], f"tools set switches that nothing reads: {dead}"
