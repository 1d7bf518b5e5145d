"""`vs_beam_topk` where its dispatch turns, against fp64 (the rule of docs/gpt2_ops_parity.md):
`e32` = the numpy fp32 restatement of the step's scoring rules against the same restatement in fp64,
max-norm relative over a shape's finite values; the kernel's finite values hold `err <= 16 * e32`, its
-inf pattern and its indices equal the restatement's.  Logits lie on a 0.25 grid and `unk_penalty` = 0.3
off it, so equal logits give bit-equal scores and distinct ones differ by >= 1e-3 in fp64
(tests/test_beam_step_ref.py asserts that for every input here): index equality is decidable.

Every shape is called with a workspace (sliced into 2048-token slices where V > 2048 and slices * k <=
1024) and without one (one block per row); both forms must give equal indices.  Rows come in eight kinds
(tests/beam_cases.py::topk_inputs): ties across a 256-lane and a slice boundary, a NaN logit, a forced
token, forced == pad, cum = -inf (all -inf, indices 0, 1, 2, ...), fewer finite entries than k, plain.
`pytest -s` prints the PARITY table of docs/beam_search_parity.md."""
import numpy as np
import pytest
import torch

import beam_cases as C

pytestmark = pytest.mark.gpu


def _kernel(xd, cumd, forcedd, k, pad, eos, unk, T, flags, workspace):
    from vidsitu_amd import _lib, ops

    rows, V = xd.shape
    val = torch.full((rows, k), 55.0, dtype=torch.float32, device=xd.device)
    idx = torch.full((rows, k), -1, dtype=torch.int64, device=xd.device)
    ws = None
    if workspace:
        ws = torch.empty(int(_lib.load().vs_beam_topk_workspace_bytes(rows, V, k)), dtype=torch.uint8,
                         device=xd.device)
    _lib.call("vs_beam_topk", ops._ptr(xd), ops._ptr(cumd), ops._ptr(forcedd), ops._ptr(val), ops._ptr(idx), rows,
              V, k, pad, eos, unk, C.UNK_PENALTY, T, flags, ops._ptr(ws), 0 if ws is None else ws.numel(),
              ops._stream())
    return val.cpu().numpy(), idx.cpu().numpy()


def _check_shape(V, k, rows, total, dev):
    x, cum, forced, pad, eos, unk = C.topk_inputs(V, total)
    xd, cumd, forcedd = (torch.from_numpy(a).to(dev) for a in (x, cum, forced))
    for T in C.TOPK_T:
        num32 = den = 0.0
        num = {True: 0.0, False: 0.0}
        for flags in (0, 1, 2):
            v64, i64 = C.topk_reference(x, cum, forced, pad, eos, unk, T, flags, np.float64, k)
            v32, i32 = C.topk_reference(x, cum, forced, pad, eos, unk, T, flags, np.float32, k)
            assert np.array_equal(i32, i64) and np.array_equal(np.isneginf(v32), np.isneginf(v64))
            dead = np.isneginf(v64).all(1)
            assert np.array_equal(i64[dead], np.tile(np.arange(k), (int(dead.sum()), 1)))
            fin = np.isfinite(v64)
            den = max(den, float(np.abs(v64[fin]).max()))
            num32 = max(num32, float(np.abs(v32[fin] - v64[fin]).max()))
            got = {}
            for workspace in (True, False):
                parts = [_kernel(xd[r: r + rows], cumd[r: r + rows], forcedd[r: r + rows], k, pad, eos, unk, T,
                                 flags, workspace) for r in range(0, total, rows)]
                v, i = (np.concatenate([p[j] for p in parts]) for j in (0, 1))
                what = f"V {V} k {k} rows {rows} T {T} flags {flags} workspace {workspace}"
                assert np.array_equal(i, i64), what
                assert np.array_equal(np.isneginf(v), np.isneginf(v64)) and not np.isnan(v).any(), what
                num[workspace] = max(num[workspace], float(np.abs(v[fin] - v64[fin]).max()))
                got[workspace] = i
            assert np.array_equal(got[True], got[False])
        e32, err_ws, err_1b = num32 / den, num[True] / den, num[False] / den
        print(f"PARITY | `beam_topk V{V} k{k} rows{rows} T{T}` | {e32:.3e} | {err_ws:.3e} | {err_1b:.3e} |")
        assert err_ws <= 16 * e32 and err_1b <= 16 * e32, (V, k, rows, T, e32, err_ws, err_1b)


@pytest.mark.parametrize("V", C.TOPK_V)
def test_beam_topk_small_vocabularies_and_slice_edges(V, dev):
    for k, rows, total in C.topk_shapes(V):
        _check_shape(V, k, rows, total, dev)


@pytest.mark.parametrize("V,k", C.TOPK_BIG)
def test_beam_topk_where_the_sliced_plan_ends(V, k, dev):
    """k = 32 at V = 65536: 32 slices * 32 = 1024 candidates, still sliced; at V = 65537: 33 slices, one
    block per row whatever the workspace; k = 31 there: 1023, sliced again.  Two rows per call."""
    _check_shape(V, k, 2, C.SPECIALS, dev)
