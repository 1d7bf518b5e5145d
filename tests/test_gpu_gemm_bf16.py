"""The MFMA GEMM of the dense projections (csrc/gemm_nt.hip), one kernel text behind two operand modes, at every edge of
its dispatch.  bf16 (vs_gemm_nt_bf16_ws, the GPT-2 decoder's mixed-precision mode): y = act(x w^T + b) + res with x, w
fp32 in memory, rounded to bf16 (nearest, ties to even) inside the kernel, multiplied on v_mfma_f32_32x32x16_bf16 with
fp32 accumulators.  f32 (vs_gemm_nt_f32_ws above 64 rows): the same loader, split rule and epilogue around
v_mfma_f32_32x32x2_f32; its tests are the `test_gemm_f32_*` twins of the bf16 ones, on shapes with M > 64 (fewer rows
never reach this kernel), and its restatement has no rounding.

Reference: both operands rounded with `tensor.bfloat16()` on the CPU, then act(x w^T + b) + res in fp64; `e32` is the
same restatement in fp32.  Rule of tests/test_gpu_gpt2_ops.py: err <= min(16 * e32, 2e-4), both relative to
max |fp64|.  It carries over because bf16 x bf16 products are exact in fp32: the kernel differs from the restatement
by fp32 summation order only.  The operands reach the kernel UNROUNDED, so a truncating or round-half-away
conversion fails by value.  With at most one non-zero product per output the result is compared bit for bit.

The kernel's k-tile is 32 wide and its split rule is `gemm_split` of the fp32 kernel, so the shapes are the ones that
rule was written for.  Every call writes into a view of a NaN-filled buffer with guard elements either side, runs with
a NaN-filled split-K workspace, and runs twice.  Every figure is printed (`PARITY ...`) before it is asserted."""
import ctypes
import functools

import pytest
import torch

from test_gpu_gpt2_ops import NAN, _bits, _check, _gen

pytestmark = pytest.mark.gpu

GUARD = 64
ACT_NAMES = {0: "none", 1: "relu", 2: "gelu_new"}


def _gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)))


MODES = {  # operand mode -> (workspace-size query, entry point)
    "bf16": ("vs_gemm_nt_bf16_workspace_bytes", "vs_gemm_nt_bf16_ws"),
    "f32": ("vs_gemm_nt_f32_workspace_bytes", "vs_gemm_nt_f32_ws"),
}


def _restate(x, w, b, res, act, dtype, mode="bf16"):
    """act(bf16(x) bf16(w)^T + b) + res evaluated in `dtype` on the CPU; mode "f32": the operands as they are."""
    if mode == "bf16":
        x, w = x.bfloat16(), w.bfloat16()
    y = x.to(dtype) @ w.to(dtype).t()
    if b is not None:
        y = y + b.to(dtype)
    if act == 1:
        y = torch.relu(y)
    elif act == 2:
        y = _gelu_new(y)
    return y if res is None else y + res.to(dtype)


@functools.lru_cache(maxsize=None)
def _case(m, n, k, act=0, bias=False, res=False, mode="bf16"):
    g = _gen(m * 1000003 + n * 1009 + k)
    x, w = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g)
    b = torch.randn(n, generator=g) if bias else None
    r = torch.randn(m, n, generator=g) if res else None
    return x, w, b, r, _restate(x, w, b, r, act, torch.float64, mode), _restate(x, w, b, r, act, torch.float32, mode)


def _run_abi(dev, x_d, w_d, b_d, r_d, act, workspace=True, mode="bf16"):
    """The mode's `_ws` entry into a guarded NaN-filled output, NaN-filled workspace.  -> y (a view), whether split."""
    from vidsitu_amd import ops

    (m, k), n = x_d.shape, w_d.shape[0]
    size_fn, entry = MODES[mode]
    need = getattr(ops._lib.load(), size_fn)(m, n, k) if workspace else 0
    ws = None
    if need:
        ws = torch.full((need // 4,), NAN, device=dev)
    buf = torch.full((m * n + 2 * GUARD,), NAN, device=dev)
    y = buf[GUARD:GUARD + m * n].view(m, n)
    ops._lib.call(entry, ops._ptr(x_d), ops._ptr(w_d), ops._ptr(b_d), ops._ptr(r_d), ops._ptr(y), m, n, k,
                  int(act), ops._ptr(ws), ctypes.c_size_t(need), ops._stream())
    assert bool(torch.isfinite(y).all()), "an output element has no owner, or the NaN workspace / LDS was read"
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + m * n:]).all()), "wrote outside y"
    return y, need > 0


def _to(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


# (M, N, K, act, expects a split-K workspace)
SHAPES = [
    (1, 1, 1, 0, False), (3, 5, 7, 0, False),  # below every tile, K % 4 != 0: the scalar loader
    (64, 64, 32, 0, False),                    # exactly one tile and one k-tile
    (65, 65, 33, 0, False),                    # one past every edge
    (65, 64, 512, 0, True),                    # split-K through the workspace (4 slices of 4 k-tiles)
    (65, 64, 2080, 0, True),                   # 16 slices asked for, 13 own a k-tile (5 each), the last one short
    (2048, 2048, 64, 0, False), (2049, 2040, 72, 0, False),  # 128x128 tiles, full and ragged
    (1024, 4096, 600, 0, False),               # a dW shape on the 128x128 path with a K tail
    (600, 1024, 1024, 0, True), (600, 4096, 1024, 2, False), (600, 1024, 4096, 0, True),  # the workload's projections
    (600, 8236, 1024, 0, False),               # an lm_head slice wide enough for the 128x128 path
]


# The fp32 arm: M > 64 only.  The same edges as above, plus three row tiles with a K tail of 8 under the split
# (130, 64, 520: 17 k-tiles in 4 slices of 5, the last slice 2 with a quarter k-tile at the end).
SHAPES_F32 = [
    (65, 65, 33, 0, False), (65, 64, 512, 0, True), (65, 64, 2080, 0, True), (130, 64, 520, 0, True),
    (2049, 2040, 72, 0, False), (1024, 4096, 600, 0, False), (600, 1024, 1024, 0, True),
]


def _shape_ids(shapes):
    return [f"M{s[0]}_N{s[1]}_K{s[2]}_{ACT_NAMES[s[3]]}" for s in shapes]


def _values(mode, m, n, k, act, split, dev):
    x, w, _, _, ref64, ref32 = _case(m, n, k, act, mode=mode)
    x_d, w_d = _to(dev, x, w)
    y, did_split = _run_abi(dev, x_d, w_d, None, None, act, mode=mode)
    assert did_split == split, "the shape no longer takes the path it was chosen for"
    _check(f"gemm_nt_{mode} M={m} N={n} K={k} act={ACT_NAMES[act]}", y, ref64, ref32)
    again, _ = _run_abi(dev, x_d, w_d, None, None, act, mode=mode)
    assert torch.equal(_bits(y), _bits(again)), "two runs differ"


@pytest.mark.parametrize("m,n,k,act,split", SHAPES, ids=_shape_ids(SHAPES))
def test_gemm_bf16_values(m, n, k, act, split, dev):
    _values("bf16", m, n, k, act, split, dev)


@pytest.mark.parametrize("m,n,k,act,split", SHAPES_F32, ids=_shape_ids(SHAPES_F32))
def test_gemm_f32_values(m, n, k, act, split, dev):
    _values("f32", m, n, k, act, split, dev)


def _no_workspace(mode, dev):
    m, n, k = 65, 64, 512
    x, w, _, _, ref64, ref32 = _case(m, n, k, mode=mode)
    x_d, w_d = _to(dev, x, w)
    y, did_split = _run_abi(dev, x_d, w_d, None, None, 0, workspace=False, mode=mode)
    assert not did_split
    _check(f"gemm_nt_{mode} M={m} N={n} K={k} no workspace", y, ref64, ref32)
    again, _ = _run_abi(dev, x_d, w_d, None, None, 0, workspace=False, mode=mode)
    assert torch.equal(_bits(y), _bits(again))


def test_gemm_bf16_split_shape_without_a_workspace_runs_unsplit(dev):
    _no_workspace("bf16", dev)


def test_gemm_f32_split_shape_without_a_workspace_runs_unsplit(dev):
    _no_workspace("f32", dev)


def _off_grid(mode, m, n, k, which, dev):
    x, w, _, _, ref64, ref32 = _case(m, n, k, mode=mode)

    def shifted(t):
        flat = torch.empty(t.numel() + 4, device=dev)
        v = flat[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v

    x_d = shifted(x) if which == "x" else x.to(dev)
    w_d = shifted(w) if which == "w" else w.to(dev)
    y, _ = _run_abi(dev, x_d, w_d, None, None, 0, mode=mode)
    _check(f"gemm_nt_{mode} M={m} N={n} K={k} {which} off the 16-byte grid", y, ref64, ref32)
    aligned, _ = _run_abi(dev, x.to(dev), w.to(dev), None, None, 0, mode=mode)
    assert torch.equal(_bits(y), _bits(aligned)), "the scalar and the 16-byte loader feed the same tiles"


OFF_GRID = dict(argnames="m,n,k", argvalues=[(65, 65, 64), (65, 64, 512)], ids=["unsplit", "split"])


@pytest.mark.parametrize("which", ["x", "w"])
@pytest.mark.parametrize(**OFF_GRID)
def test_gemm_bf16_pointer_off_the_16_byte_grid_takes_the_scalar_loader(m, n, k, which, dev):
    _off_grid("bf16", m, n, k, which, dev)


@pytest.mark.parametrize("which", ["x", "w"])
@pytest.mark.parametrize(**OFF_GRID)
def test_gemm_f32_pointer_off_the_16_byte_grid_takes_the_scalar_loader(m, n, k, which, dev):
    _off_grid("f32", m, n, k, which, dev)


def _epilogue(mode, m, n, k, act, dev):
    """Bias, act, res and out= all given: through the C ABI with sentinels, and through ops.gemm_nt(bf16=...)."""
    from vidsitu_amd import ops

    bf16 = mode == "bf16"
    x, w, b, r, ref64, ref32 = _case(m, n, k, act, True, True, mode)
    x_d, w_d, b_d, r_d = _to(dev, x, w, b, r)
    y, did_split = _run_abi(dev, x_d, w_d, b_d, r_d, act, mode=mode)
    assert did_split == (k == 512)
    name = f"gemm_nt_{mode} M={m} N={n} K={k} bias act={ACT_NAMES[act]} res"
    _check(name, y, ref64, ref32)
    out = torch.full((m, n), NAN, device=dev)
    got = ops.gemm_nt(x_d, w_d, b_d, r_d, act=act, out=out, bf16=bf16)
    assert got is out and torch.equal(_bits(out), _bits(y)), f"ops.gemm_nt(bf16={bf16}) is the same launch"
    # each part alone is what it says
    for nm, bb, rr in (("bias", b, None), ("res", None, r)):
        got = ops.gemm_nt(x_d, w_d, None if bb is None else b_d, None if rr is None else r_d, act=act, bf16=bf16)
        _check(f"gemm_nt_{mode} M={m} N={n} K={k} act={ACT_NAMES[act]} {nm} only", got,
               _restate(x, w, bb, rr, act, torch.float64, mode), _restate(x, w, bb, rr, act, torch.float32, mode))


EPILOGUE = dict(argnames="m,n,k", argvalues=[(65, 65, 33), (65, 64, 512)], ids=["unsplit", "split"])


@pytest.mark.parametrize("act", [0, 1, 2], ids=[ACT_NAMES[a] for a in (0, 1, 2)])
@pytest.mark.parametrize(**EPILOGUE)
def test_gemm_bf16_epilogue(m, n, k, act, dev):
    _epilogue("bf16", m, n, k, act, dev)


@pytest.mark.parametrize("act", [0, 1, 2], ids=[ACT_NAMES[a] for a in (0, 1, 2)])
@pytest.mark.parametrize(**EPILOGUE)
def test_gemm_f32_epilogue(m, n, k, act, dev):
    _epilogue("f32", m, n, k, act, dev)


def test_gemm_bf16_flag_off_is_the_fp32_path(dev):
    from vidsitu_amd import ops

    x, w, _, _, _, _ = _case(65, 64, 512)
    x_d, w_d = _to(dev, x, w)
    plain, flagged, on = ops.gemm_nt(x_d, w_d), ops.gemm_nt(x_d, w_d, bf16=False), ops.gemm_nt(x_d, w_d, bf16=True)
    assert torch.equal(_bits(plain), _bits(flagged)) and not torch.equal(_bits(plain), _bits(on))


# ---------------------------------------------------------------------------------------------
# exact cases: at most one non-zero product per output
# ---------------------------------------------------------------------------------------------
TIES = [1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8]                       # -> 1 and 1 + 2^-6 (ties to even)
PROBES = TIES + [t + s * 2.0 ** -23 for t in TIES for s in (-1, 1)]      # and the fp32 neighbours of both ties
PROBES = PROBES + [-v for v in PROBES]
ROUNDED = [1.0, 1 + 2.0 ** -6, 1.0, 1 + 2.0 ** -7, 1 + 2.0 ** -7, 1 + 2.0 ** -6]
ROUNDED = ROUNDED + [-v for v in ROUNDED]


def _with_probes(t, g):
    """Random values with the tie probes scattered over every row."""
    flat = t.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:max(len(PROBES), flat.numel() // 3)]
    flat[idx] = torch.tensor(PROBES, dtype=torch.float32).repeat(idx.numel() // len(PROBES) + 1)[:idx.numel()]
    return t


def test_probe_values_round_as_stated():
    v = torch.tensor(PROBES, dtype=torch.float32)
    assert v.double().tolist() == PROBES and v.bfloat16().float().tolist() == ROUNDED


@pytest.mark.parametrize("m,n", [(1, 1), (12, 1), (70, 130)])
def test_gemm_bf16_k1_is_the_product_of_the_rounded_operands_bit_for_bit(m, n, dev):
    """K = 1 (the scalar loader): y[i, j] = fp32(bf16(x[i])) * fp32(bf16(w[j])), with the tie probes on every second
    row of x and every third of w.  The 128x128 kernel and the split are covered by the one-hot case below."""
    g = _gen(m + n)
    probes = torch.tensor(PROBES, dtype=torch.float32)
    x, w = torch.randn(m, 1, generator=g), torch.randn(n, 1, generator=g)
    x[::2, 0] = probes.repeat(m)[:x[::2].shape[0]]
    w[::3, 0] = probes.flip(0).repeat(n)[:w[::3].shape[0]]
    want = x.bfloat16().float() * w.bfloat16().float().t()
    y, _ = _run_abi(dev, x.to(dev), w.to(dev), None, None, 0)
    assert torch.equal(_bits(y).cpu(), _bits(want))
    if m == 1 and n == 1:  # (1 + 2^-8) * -(1 + 2^-7 + 2^-8 + 2^-23): 1 * -(1 + 2^-6)
        assert float(y) == -(1 + 2.0 ** -6)


@pytest.mark.parametrize("m,n,k", [(70, 70, 40), (65, 64, 512), (2048, 2048, 72), (33, 9, 77)],
                         ids=["unsplit", "split", "t128", "scalar_loader"])
def test_gemm_bf16_one_hot_rows_of_w_select_rounded_products_bit_for_bit(m, n, k, dev):
    """Row j of w holds one non-zero at column c(j): y[i, j] = fp32(bf16(x[i, c(j)])) * fp32(bf16(w[j, c(j)])) exactly
    (a product of two bf16 values has 16 significant bits; adding zeros changes nothing), through the split-K reduce
    too."""
    g = _gen(k)
    x = _with_probes(torch.randn(m, k, generator=g), g)
    x[x == 0] = 1.0
    col = torch.randint(0, k, (n,), generator=g)
    col[:min(n, k)] = torch.randperm(k, generator=g)[:min(n, k)]  # every k-tile and the K tail are hit
    val = _with_probes(torch.randn(n, generator=g), g)
    w = torch.zeros(n, k)
    w[torch.arange(n), col] = val
    want = x.bfloat16().float()[:, col] * val.bfloat16().float()[None, :]
    y, _ = _run_abi(dev, x.to(dev), w.to(dev), None, None, 0)
    assert torch.equal(_bits(y).cpu(), _bits(want))
