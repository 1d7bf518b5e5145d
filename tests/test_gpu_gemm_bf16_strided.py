"""The K-strided operand forms of the bf16 MFMA GEMM (csrc/gemm_nt.hip: GemmBf16T, vs_gemm_bf16_ws, ops.gemm_bf16):
an operand stored [K][rows] is transposed inside the loader on its way into LDS.

The tile the strided loader leaves is byte for byte the tile the K-contiguous loader leaves for the transposed copy,
and everything behind the tile store is shared code, so the first rule is BITWISE equality (`torch.equal`) with
`ops.gemm_nt(transpose_f32(a), transpose_f32(b), bf16=True)` at the same M, N, K and with the workspace `ops` provides:
any difference is a loader bug.  The second rule is the project's bf16 rule against the fp64 restatement of
tests/test_gpu_gemm_bf16.py (operands rounded with `tensor.bfloat16()`): err <= min(16 * e32, 2e-4).

Shapes, each under (a_t, b_t) = (0, 1), (1, 0), (1, 1):
  65 x 67 x 70        unsplit 64 x 64 tiles, every edge ragged: rows no multiple of 4 (scalar row loads), K no multiple
                      of 32 nor of 2 (the last k-pair is half outside)
  64 x 64 x 1, 31, 33 K below one pair, below one k-tile, one past it
  80 x 3072 x 768, 600 x 1024 x 1024   split-K slabs (gemm_split > 1)
  2048 x 2048 x 70    128 x 128 tiles
Every call through the C ABI writes into a view of a NaN-filled buffer with guard elements either side and gets a
NaN-filled workspace with guards behind it.  Every figure is printed (`PARITY ...`) before it is asserted."""
import ctypes
import functools

import pytest
import torch

from test_gpu_gemm_bf16 import ACT_NAMES, GUARD, _restate
from test_gpu_gpt2_ops import NAN, _bits, _check, _gen

pytestmark = pytest.mark.gpu

FLAGS = [(0, 1), (1, 0), (1, 1)]
FLAG_IDS = ["a_k_b_t", "a_t_b_k", "a_t_b_t"]
# (M, N, K, split-K expected)
SHAPES = [(65, 67, 70, False), (64, 64, 1, False), (64, 64, 31, False), (64, 64, 33, False),
          (80, 3072, 768, True), (600, 1024, 1024, True), (2048, 2048, 70, False)]
SHAPE_IDS = [f"M{m}_N{n}_K{k}" for m, n, k, _ in SHAPES]


@functools.lru_cache(maxsize=None)
def _case(m, n, k, act=0, bias=False, res=False):
    """Logical operands A [M, K], B [N, K] and the fp64 / fp32 restatements: computed once, left unchanged."""
    g = _gen(m * 1000003 + n * 1009 + k + 17)
    a, b = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g)
    bb = torch.randn(n, generator=g) if bias else None
    r = torch.randn(m, n, generator=g) if res else None
    return a, b, bb, r, _restate(a, b, bb, r, act, torch.float64), _restate(a, b, bb, r, act, torch.float32)


def _stored(t, strided, dev):
    """The operand as the form wants it in memory: [rows][K], or [K][rows] for a strided one."""
    return (t.t().contiguous() if strided else t).to(dev)


def _nt_reference(a_s, b_s, a_t, b_t, bias, res, act):
    """The NT form on transposed copies, through ops (its workspace, its split)."""
    from vidsitu_amd import ops

    return ops.gemm_nt(ops.transpose_f32(a_s) if a_t else a_s, ops.transpose_f32(b_s) if b_t else b_s, bias, res,
                       act=act, bf16=True)


def _run_abi(dev, a_s, b_s, m, n, k, a_t, b_t, bias=None, res=None, act=0):
    """vs_gemm_bf16_ws into a guarded NaN-filled output with a guarded NaN-filled workspace.  -> y, whether split."""
    from vidsitu_amd import ops

    need = ops._lib.load().vs_gemm_nt_bf16_workspace_bytes(m, n, k)
    wsbuf = torch.full((need // 4 + 2 * GUARD,), NAN, device=dev)
    ws = wsbuf[GUARD:GUARD + need // 4] if need else None
    buf = torch.full((m * n + 2 * GUARD,), NAN, device=dev)
    y = buf[GUARD:GUARD + m * n].view(m, n)
    ops._lib.call("vs_gemm_bf16_ws", ops._ptr(a_s), ops._ptr(b_s), ops._ptr(bias), ops._ptr(res), ops._ptr(y), m, n, k,
                  int(a_t), int(b_t), int(act), ops._ptr(ws), ctypes.c_size_t(need), ops._stream())
    assert bool(torch.isfinite(y).all()), "an output element has no owner, or the NaN workspace / LDS was read"
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + m * n:]).all()), "wrote outside y"
    assert bool(torch.isnan(wsbuf[:GUARD]).all()) and bool(torch.isnan(wsbuf[GUARD + need // 4:]).all()), \
        "wrote outside the slabs"
    return y, need > 0


@pytest.mark.parametrize("a_t,b_t", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("m,n,k,split", SHAPES, ids=SHAPE_IDS)
def test_strided_forms_equal_the_nt_form_on_transposed_copies_bit_for_bit(m, n, k, split, a_t, b_t, dev):
    from vidsitu_amd import ops

    a, b, _, _, ref64, ref32 = _case(m, n, k)
    a_s, b_s = _stored(a, a_t, dev), _stored(b, b_t, dev)
    want = _nt_reference(a_s, b_s, a_t, b_t, None, None, 0)
    y, did_split = _run_abi(dev, a_s, b_s, m, n, k, a_t, b_t)
    assert did_split == split, "the shape no longer takes the path it was chosen for"
    name = f"gemm_bf16 a_t={a_t} b_t={b_t} M={m} N={n} K={k}"
    diff = int((_bits(y) != _bits(want)).sum())
    print(f"PARITY {name} elements that differ from the NT form: {diff} of {m * n}")
    _check(name, y, ref64, ref32)
    assert diff == 0 and torch.equal(y, want)
    got = ops.gemm_bf16(a_s, b_s, a_t=bool(a_t), b_t=bool(b_t))
    assert torch.equal(_bits(got), _bits(want)), "ops.gemm_bf16 is the same launch"
    again, _ = _run_abi(dev, a_s, b_s, m, n, k, a_t, b_t)
    assert torch.equal(_bits(y), _bits(again)), "two runs differ"


def test_both_flags_off_is_the_nt_entry(dev):
    from vidsitu_amd import ops

    for m, n, k in ((65, 67, 70), (80, 3072, 768)):
        a, b, _, _, ref64, ref32 = _case(m, n, k)
        a_d, b_d = a.to(dev), b.to(dev)
        y, _ = _run_abi(dev, a_d, b_d, m, n, k, 0, 0)
        assert torch.equal(_bits(y), _bits(ops.gemm_nt(a_d, b_d, bf16=True)))
        assert torch.equal(_bits(ops.gemm_bf16(a_d, b_d)), _bits(y))
        _check(f"gemm_bf16 a_t=0 b_t=0 M={m} N={n} K={k}", y, ref64, ref32)


@pytest.mark.parametrize("a_t,b_t", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("which", ["a", "b"])
def test_a_base_off_the_16_byte_grid_takes_the_scalar_loader(which, a_t, b_t, dev):
    """Rows a multiple of 4 (the aligned call takes 16-byte loads), one operand 4 bytes off the grid: same bits, no
    fault."""
    m, n, k = 64, 68, 40
    a, b, _, _, ref64, ref32 = _case(m, n, k)
    a_s, b_s = _stored(a, a_t, dev), _stored(b, b_t, dev)

    def shifted(t):
        flat = torch.empty(t.numel() + 4, device=dev)
        v = flat[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v

    aligned, _ = _run_abi(dev, a_s, b_s, m, n, k, a_t, b_t)
    y, _ = _run_abi(dev, shifted(a_s) if which == "a" else a_s, shifted(b_s) if which == "b" else b_s, m, n, k, a_t, b_t)
    _check(f"gemm_bf16 a_t={a_t} b_t={b_t} M={m} N={n} K={k} {which} off the 16-byte grid", y, ref64, ref32)
    assert torch.equal(_bits(y), _bits(aligned)), "the scalar and the 16-byte loader feed the same tiles"
    assert torch.equal(_bits(y), _bits(_nt_reference(a_s, b_s, a_t, b_t, None, None, 0)))


EPILOGUES = [("bias", 0, True, False), ("res", 0, False, True), ("relu", 1, True, False),
             ("gelu_new", 2, True, True), ("all", 1, True, True)]


@pytest.mark.parametrize("m,n,k", [(65, 67, 70), (80, 3072, 768)], ids=["unsplit", "split"])
@pytest.mark.parametrize("what,act,bias,res", EPILOGUES, ids=[e[0] for e in EPILOGUES])
def test_epilogue_through_the_new_entry(what, act, bias, res, m, n, k, dev):
    from vidsitu_amd import ops

    a, b, bb, r, ref64, ref32 = _case(m, n, k, act, bias, res)
    for a_t, b_t in FLAGS:
        a_s, b_s = _stored(a, a_t, dev), _stored(b, b_t, dev)
        b_d, r_d = (None if t is None else t.to(dev) for t in (bb, r))
        y, _ = _run_abi(dev, a_s, b_s, m, n, k, a_t, b_t, b_d, r_d, act)
        _check(f"gemm_bf16 a_t={a_t} b_t={b_t} M={m} N={n} K={k} {what} act={ACT_NAMES[act]}", y, ref64, ref32)
        assert torch.equal(_bits(y), _bits(_nt_reference(a_s, b_s, a_t, b_t, b_d, r_d, act)))
        out = torch.full((m, n), NAN, device=dev)
        got = ops.gemm_bf16(a_s, b_s, b_d, r_d, act=act, out=out, a_t=bool(a_t), b_t=bool(b_t))
        assert got is out and torch.equal(_bits(out), _bits(y)), "out= is written in place by the same launch"


@pytest.mark.parametrize("d,t", [(64, 69), (66, 69), (768, 80)], ids=["D64_T69", "D66_T69_off_grid", "D768_T80"])
def test_a_column_range_of_an_array_is_a_strided_operand(d, t, dev):
    """The three weight gradients of a fused q|k|v projection: dW_s = dqkv[:, s*D:(s+1)*D]^T . x, read in place with
    the array's leading dimension.  D = 66: the ranges start 8 bytes off the 16-byte grid (scalar loads)."""
    from vidsitu_amd import ops

    g = _gen(d + t)
    dqkv, x = torch.randn(t, 3 * d, generator=g), torch.randn(t, d, generator=g)
    dqkv_d, x_d = dqkv.to(dev), x.to(dev)
    dqkv_t, x_t = ops.transpose_f32(dqkv_d), ops.transpose_f32(x_d)
    for s in range(3):
        sl = slice(s * d, (s + 1) * d)
        out = torch.full((d, d), NAN, device=dev)
        got = ops.gemm_bf16(dqkv_d[:, sl], x_d, out=out, a_t=True, b_t=True)
        want = ops.gemm_nt(dqkv_t[sl], x_t, bf16=True)
        a, b = dqkv[:, sl].t().contiguous(), x.t().contiguous()
        _check(f"gemm_bf16 column range {s} D={d} T={t}", got, _restate(a, b, None, None, 0, torch.float64),
               _restate(a, b, None, None, 0, torch.float32))
        assert got is out and torch.equal(_bits(got), _bits(want))
        # and as the B operand
        got = ops.gemm_bf16(x_d, dqkv_d[:, sl], a_t=True, b_t=True)
        assert torch.equal(_bits(got), _bits(ops.gemm_nt(x_t, dqkv_t[sl], bf16=True)))


def test_bad_arguments_return_a_negative_status_and_launch_nothing(dev):
    from vidsitu_amd import ops

    lib = ops._lib.load()
    m, n, k = 80, 3072, 768
    a, b, *_ = _case(m, n, k)
    a_d, b_s = a.to(dev), _stored(b, 1, dev)
    need = lib.vs_gemm_nt_bf16_workspace_bytes(m, n, k)
    assert need > 0
    ws = torch.full((need // 4,), 7.0, device=dev)
    y = torch.full((m, n), 7.0, device=dev)
    p = ops._ptr
    size = ctypes.c_size_t
    torch.cuda.synchronize()
    before = lib.vs_launch_count()
    st = ops._stream()
    calls = {
        "a null": (None, p(b_s), None, None, p(y), m, n, k, 0, 1, 0, p(ws), size(need), st),
        "b null": (p(a_d), None, None, None, p(y), m, n, k, 0, 1, 0, p(ws), size(need), st),
        "y null": (p(a_d), p(b_s), None, None, None, m, n, k, 0, 1, 0, p(ws), size(need), st),
        "M = 0": (p(a_d), p(b_s), None, None, p(y), 0, n, k, 0, 1, 0, p(ws), size(need), st),
        "N < 0": (p(a_d), p(b_s), None, None, p(y), m, -n, k, 0, 1, 0, p(ws), size(need), st),
        "K = 0": (p(a_d), p(b_s), None, None, p(y), m, n, 0, 0, 1, 0, p(ws), size(need), st),
        "act = 3": (p(a_d), p(b_s), None, None, p(y), m, n, k, 0, 1, 3, p(ws), size(need), st),
        "act = -1": (p(a_d), p(b_s), None, None, p(y), m, n, k, 0, 1, -1, p(ws), size(need), st),
        "flag = 2": (p(a_d), p(b_s), None, None, p(y), m, n, k, 0, 2, 0, p(ws), size(need), st),
        "short workspace": (p(a_d), p(b_s), None, None, p(y), m, n, k, 0, 1, 0, p(ws), size(need - 4), st),
        "no workspace": (p(a_d), p(b_s), None, None, p(y), m, n, k, 0, 1, 0, None, size(0), st),
    }
    for name, args in calls.items():
        rc = lib.vs_gemm_bf16_ws(*args)
        print(f"vs_gemm_bf16_ws {name}: status {rc} ({lib.vs_last_error_string().decode()})")
        assert rc < 0, name
    assert lib.vs_launch_count() == before
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((ws == 7.0).all())


def test_ops_gemm_bf16_checks_shapes(dev):
    from vidsitu_amd import ops

    a, b = torch.zeros(8, 12, device=dev), torch.zeros(16, 12, device=dev)
    bad = [
        dict(a=a, b=torch.zeros(16, 13, device=dev)),                      # K mismatch, both K-contiguous
        dict(a=a, b=b, a_t=True),                                          # a read as [K=8][M=12] against K = 12
        dict(a=a, b=b, b_t=True),                                          # b read as [K=16][N=12]
        dict(a=a, b=b, bias=torch.zeros(15, device=dev)),
        dict(a=a, b=b, res=torch.zeros(8, 15, device=dev)),
        dict(a=a, b=b, out=torch.zeros(16, 8, device=dev)),
        dict(a=a.view(2, 4, 12), b=b),
        dict(a=a.double(), b=b),
    ]
    for kw in bad:
        with pytest.raises(ops._lib.VsError):
            ops.gemm_bf16(**kw)
    assert ops.gemm_bf16(a.t().contiguous(), b.t().contiguous(), a_t=True, b_t=True).shape == (8, 16)
