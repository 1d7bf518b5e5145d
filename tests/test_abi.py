"""The C-ABI library loads without a GPU and exports every symbol include/vidsitu_hip.h
declares (no compute calls here)."""
import ctypes
import os
import re

from vidsitu_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    hdr = open(os.path.join(ROOT, "include", "vidsitu_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(vs_[a-z0-9_]+)\s*\(", hdr))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    names = _header_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in the header but not exported"
    assert names == set(_lib.SIGNATURES), "python binding table out of sync with the header"


def test_version_and_error_string():
    lib = _lib.load()
    assert lib.vs_version() >= 1
    assert isinstance(lib.vs_last_error_string(), bytes)


def test_conv_desc_layout_matches_header():
    assert ctypes.sizeof(_lib.ConvDesc) == 22 * 4
    hdr = open(os.path.join(ROOT, "include", "vidsitu_hip.h")).read()
    body = re.search(r"typedef struct vs_conv_desc \{(.*?)\} vs_conv_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in re.findall(r"int32_t ([^;]+);", body):
        fields += [f.strip() for f in decl.split(",")]
    assert fields == [f[0] for f in _lib.ConvDesc._fields_]


def test_argument_validation_without_gpu():
    """Bad descriptors are rejected on the host before any launch."""
    lib = _lib.load()
    d = _lib.ConvDesc()
    d.N, d.Cin, d.Cout = 1, 3, 8  # Cin not a multiple of 8
    rc = lib.vs_conv_fwd(None, None, None, ctypes.byref(d), None, None, None, None, None, 0, None)
    assert rc == -1
    assert b"multiples of 8" in lib.vs_last_error_string()


def test_flag_constants_follow_the_header():
    """Every `#define VS_CONV_* (1 << n)` / `VS_WGRAD_*` of the header equals the Python constant of the same name, and
    the two function-like macros encode what their Python namesakes do."""
    hdr = open(os.path.join(ROOT, "include", "vidsitu_hip.h")).read()
    bits = re.findall(r"#define (VS_(?:CONV|WGRAD)_[A-Z0-9_]+) \(1 << (\d+)\)", hdr)
    plain = re.findall(r"#define (VS_CONV_[A-Z0-9_]+) (\d+)\b", hdr)
    assert len(bits) >= 14 and len(plain) == 5
    for name, n in bits:
        assert getattr(_lib, name) == 1 << int(n), name
    for name, v in plain:
        assert getattr(_lib, name) == int(v), name
    assert "#define VS_CONV_TILE(id) (((id) + 1) << 8)" in hdr
    assert "#define VS_CONV_RING(ns) (((ns) & 7) << 16)" in hdr
    assert [_lib.VS_CONV_TILE(i) for i in (0, 7)] == [1 << 8, 8 << 8]
    assert [_lib.VS_CONV_RING(i) for i in (0, 1, 4, 9)] == [0, 1 << 16, 4 << 16, 1 << 16]
    # and the header defines nothing of the kind that Python lacks under another spelling
    assert {n for n, _ in bits} | {n for n, _ in plain} == {n for n in dir(_lib) if re.fullmatch(r"VS_(CONV|WGRAD)_[A-Z0-9_]+", n)
                                                       and isinstance(getattr(_lib, n), int)}
