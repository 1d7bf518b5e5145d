"""A captured eval forward that knows which folds it was captured with.

A hipGraph keeps the tensors it was recorded with: the BN folds, the bf16 weight copies.  `calibrate_weight_rounding`,
`reset_weight_rounding`, a re-fold after a running-statistic or weight change replace those tensors, and a graph captured
before goes on computing with the old ones without any sign of it.  The trunk counts such events
(`VideoTrunk.eval_version`) and knows whether a change is pending that the next eager forward would fold in
(`eval_state_version()`: a train-mode pass, an optimizer step, a `load_state_dict`); `EvalGraph` records that state at
capture and `replay()` raises `VsError` under any other.  It never recaptures on its own: the caller decides when a
new graph is worth its capture.
"""
import torch

from ._lib import VsError

FRAME_KEYS = ("frms_ev_raw_u8", "frms_ev_fast_u8")


class EvalGraph:
    """`step()` (a no-grad eval forward that reads static input tensors and returns its output tensor) warmed up,
    captured into one hipGraph and replayed; `version()` reads the counter the capture is valid for."""

    def __init__(self, step, version, warmup=2):
        self.step, self.version, self.warmup = step, version, int(warmup)
        self.captured_version = None
        self.graph = self.out = None

    # ---- the two device-side halves (a stub replaces them in the host-only test) ----
    def _capture(self):
        st = torch.cuda.current_stream()
        for _ in range(max(1, self.warmup)):  # folds, weight copies, tables, per-stream scratch: all made here
            self.step()
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        on = {} if st == torch.cuda.default_stream(st.device) else {"stream": st}
        with torch.cuda.graph(g, **on):  # on the warm-up's stream: its cached scratch buffers are re-used
            out = self.step()
        self.graph = g
        return out

    def _replay(self):
        self.graph.replay()

    # ---- the version check ----
    def capture(self):
        self.captured_version = None
        self.out = self._capture()
        self.captured_version = self.version()  # after the warm-up's own re-fold, if there was one
        return self

    def replay(self):
        """Replay on the current stream; -> the static output tensor."""
        if self.captured_version is None:
            raise VsError("EvalGraph.replay() before capture()")
        now = self.version()
        if now != self.captured_version:
            raise VsError(
                f"stale eval graph: captured at eval state {self.captured_version}, the trunk is at {now} -- its BN "
                "folds or weight copies were replaced since, or are due to be (calibrate_weight_rounding, "
                "reset_weight_rounding, a weight / running-statistic change: train-mode pass, optimizer step, "
                "load_state_dict), and a replay would still read the old ones; capture a new EvalGraph")
        self._replay()
        return self.out

    @classmethod
    def for_model(cls, mdl, batch, warmup=2):
        """Ingest -> trunk -> head of `mdl` (an eval-mode `SFBase`) for the shape of `batch` (a dict with ONE uint8 frame
        key on the GPU).  `.inp` is the static input ([B, E, T, H, W, 3] uint8: copy the next batch into it), the
        replayed output `.feats` is [B, E, C] float32.  Captures on the current stream."""
        keys = [k for k in FRAME_KEYS if k in batch]
        if len(keys) != 1:
            raise VsError(f"EvalGraph.for_model wants exactly one of {FRAME_KEYS} in the batch, got {sorted(batch)}")
        if mdl.training:
            raise VsError("EvalGraph captures the eval forward (call .eval() first)")
        inp = {keys[0]: batch[keys[0]].clone()}
        b, e = inp[keys[0]].shape[:2]

        def step():
            with torch.no_grad():
                return mdl.head(mdl.forward_encoder(inp))  # [B * E, C, 1, 1, 1] fp32

        g = cls(step, mdl.sf_mdl.eval_state_version, warmup)
        g.key, g.inp = keys[0], inp[keys[0]]
        g.capture()
        g.feats = g.out.view(b, e, -1)  # (a view: the graph's static output under the shape forward_all saves)
        return g
