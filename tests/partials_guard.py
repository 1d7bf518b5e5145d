"""The row guard on per-block partial buffers, shared by the GPU test files that use it (a plain module: import the
fixture by name into the test file)."""
import pytest
import torch


@pytest.fixture
def guarded_partials(monkeypatch):
    """A rows query and the launch it sizes a buffer for choose the same kernel.  Every [rows, 2, C] buffer of per-block
    partials that ops allocates from a rows query during the test (forward BN statistics -- the stems' included --,
    BN-backward sums of one or two units, apply on load) becomes the front of a NaN-filled buffer four rows longer.  At
    the end every float of the `rows` rows has been written and the four rows behind them are still NaN: a launch that
    chose another kernel than the query writes more rows or fewer.  The guard rows hold an overrun of up to four rows
    inside the allocation and show any longer one by its first four rows; they do not contain it (a 128-row tile kernel
    behind a query that answered for 256-row tiles writes twice the rows)."""
    from vidsitu_amd import ops

    made = []

    def partials(rows, c, device):
        full = torch.full((rows + 4, 2, c), float("nan"), dtype=torch.float32, device=device)
        made.append((full, rows))
        return full[:rows]

    monkeypatch.setattr(ops, "_partials", partials)
    yield made
    assert made, "the test allocated no partials"
    for i, (full, rows) in enumerate(made):
        assert not bool(torch.isnan(full[:rows]).any()), f"partials {i}: not every one of the {rows} rows was written"
        assert bool(torch.isnan(full[rows:]).all()), f"partials {i}: the launch wrote past the {rows} rows of the query"
