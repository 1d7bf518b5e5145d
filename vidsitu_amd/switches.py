"""Every VS_* environment variable the package reads: name -> default, kind, one line.  The library's own switches are
the table in csrc/switches.h; INTEGRATION.md ("Environment switches") lists both and tests/test_switch_list.py holds
the three to each other.  `python -m vidsitu_amd.switches` prints what each switch resolved to.

No torch and no _lib in here: _lib.py asks this module for VS_LIB_PATH.

`read(name)` parses by the switch's kind; the default is parsed by the same rule, "unset" is None:
  on     True unless the value is "0"
  off    True only if the value is "1"
  int    int(value)
  adam   VS_ADAM_OVERLAP: 0 for "0" / "", 2 for "2", 1 for anything else
  fill   VS_GRAD_FILL: False / True / "learn" for "0" / "1" / "learn", None (no override) for anything else
  text   the value itself
"""
import os
import re
from collections import namedtuple

Switch = namedtuple("Switch", "default kind meaning")

SWITCHES = {
    "VS_LIB_PATH": Switch("unset", "text", "path of the shared library to load instead of `vidsitu_amd/libvidsitu_hip.so`"),
    "VS_CKPT_UNSAFE_LOAD": Switch("unset", "text", "`1`: `load_model_dict` may unpickle a checkpoint that is not weights-only"),
    "VS_DUAL_STREAM": Switch("1", "on", "`0`: both pathways of the trunk on the caller's stream"),
    "VS_WGRAD_LANES": Switch("1", "on", "`0`: weight gradients inline instead of on the side lane"),
    "VS_CONV_PAIR": Switch("1", "on", "`0`: a unit's data gradient and weight gradient as two launches"),
    "VS_REDUCE_MERGE": Switch("1", "on", "`0`: a weight gradient's slab reduce as a launch of its own, not merged with the next BN-backward finalize"),
    "VS_FUSE_BN_SUMS": Switch("1", "on", "`0`: BN-backward sums from a reduce pass instead of the consuming dgrad's epilogue"),
    "VS_FUSE_SC_SUMS": Switch("1", "on", "`0`: the same for the shortcut unit's sums"),
    "VS_FUSE_SC_APPLY": Switch("1", "on", "`0`: the shortcut's BN apply as a pass of its own (training forward)"),
    "VS_FUSE_SC_BWD": Switch("1", "on", "`0`: the c and shortcut units' BN-backward apply as two passes"),
    "VS_FUSE_ON_FAST": Switch("1", "on", "`0`: the lateral connections on the caller's stream instead of the fast pathway's"),
    "VS_STEM_POOL_FUSE": Switch("1", "on", "`0`: the stems' BN + ReLU and max-pool as separate launches (training forward)"),
    "VS_STEM_POOL_FUSE_BWD": Switch("0", "off", "`1`: the pool's backward inside the stems' BN-backward passes"),
    "VS_WGRAD_GROUP": Switch("1", "on", "`0`: per-unit weight-gradient launches instead of one grouped launch per block"),
    "VS_WGRAD_GROUP_SPAN": Switch("3", "int", "blocks whose weight gradients share one grouped launch"),
    "VS_WGRAD_GROUP_MINC": Switch("128", "int", "narrowest output width that is grouped"),
    "VS_EVAL_FUSE_BC": Switch("1", "on", "`0`: conv b and conv c of the fast pathway as two launches (evaluation)"),
    "VS_EVAL_SPLIT_WEIGHTS": Switch("0", "off", "`1`: evaluation with split bf16 weights, two launches per convolution"),
    "VS_RESIDUAL_FP32": Switch("0", "off", "`1`: evaluation keeps a stage's identity chain in fp32"),
    "VS_BN_FIN2": Switch("1", "on", "`0`: the round-4 BN finalize launches instead of the one-launch form"),
    "VS_BN_TWO_LEVEL": Switch("512", "int", "partial rows above which a level-1 reduce runs in front of the finalize"),
    "VS_LINEAR_BWD_FUSED": Switch("1", "on", "`0`: a few-row linear's backward as three launches"),
    "VS_RESIDUAL_ROUTE": Switch("1", "on", "`0`: autograd's add for the encoder's residual gradient instead of the dgrad epilogue"),
    "VS_TRANSPOSE_LATE": Switch("1", "on", "`0`: the dgrad weight images are refreshed at the start of the step"),
    "VS_GRAD_FILL": Switch("unset", "fill", "`0` / `1` / `learn`: overrides `TrainStep`'s `grad_fill` argument"),
    "VS_ADAM_OVERLAP": Switch("0", "adam", "`1`: ranged Adam beside the backward pass (single process); `2`: every range at the end"),
    "VS_GEN_GRAPHS": Switch("1", "on", "`0`: generation without captured decode-step graphs"),
    "VS_WHATIF": Switch("0", "int", "tools only: bit mask of kernel families to skip (garbage numerics); refused without `VS_WHATIF_OK=1`"),
    "VS_WHATIF_OK": Switch("unset", "text", "`1`: the guard that lets the two `VS_WHATIF*` switches act"),
}

_PARSE = {
    "on": lambda s: s != "0",
    "off": lambda s: s == "1",
    "int": int,
    "adam": lambda s: 0 if s in ("0", "") else (2 if s == "2" else 1),
    "fill": lambda s: {"0": False, "1": True, "learn": "learn"}.get(s),
    "text": lambda s: s,
}


def read(name, env=None):
    """The value of switch `name` in `env` (default: the process environment), parsed by its kind."""
    env = os.environ if env is None else env
    sw = SWITCHES[name]
    s = env.get(name, sw.default)
    value = None if name not in env and s == "unset" else _PARSE[sw.kind](s)
    # VS_WHATIF (tools/whatif.sh: whole kernel families skipped to time what they cost -- GARBAGE numerics) is refused
    # unless the tools-only guard VS_WHATIF_OK=1 stands beside it: a leaked variable must not train silently on garbage.
    if name == "VS_WHATIF" and value != 0 and env.get("VS_WHATIF_OK") != "1":
        raise RuntimeError("VS_WHATIF skips kernel launches (garbage numerics, timing experiments only): set "
                           "VS_WHATIF_OK=1 beside it, or unset it")
    return value


def library_table():
    """name -> (C type, default as written) of the library's switches: the X(...) lines of csrc/switches.h."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "switches.h")) as f:
        rows = re.findall(r"^\s*X\((\w+), ([a-z ]+), ([-0-9.]+)\)", f.read(), re.M)
    return {"VS_" + n: (t, d) for n, t, d in rows}


def main():
    import ctypes

    from . import _lib

    lib, libsw = _lib.load(), library_table()
    for name in sorted(set(SWITCHES) | set(libsw)):
        side = "both" if name in SWITCHES and name in libsw else ("package" if name in SWITCHES else "library")
        default = SWITCHES[name].default if name in SWITCHES else libsw[name][1]
        resolved = []
        if name in SWITCHES:
            resolved.append(repr(read(name)))
        if name in libsw:
            v = ctypes.c_double()
            _lib.check(lib.vs_switch_value(name.encode(), ctypes.byref(v)), "vs_switch_value")
            resolved.append("%g" % v.value)
        print(f"{name:28s} default {default:8s} resolved {' / '.join(resolved):16s} {side}")
    for name in sorted(os.environ):
        if name.startswith("VS_") and name not in SWITCHES and name not in libsw:
            print(f"{name:28s} read by nobody in the package")


if __name__ == "__main__":
    main()
