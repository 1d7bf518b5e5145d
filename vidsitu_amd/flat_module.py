"""The host-side plumbing the GPT-2, fairseq-decoder and RoBERTa modules share ("flat-parameter hosts").

Each of those models registers its parameters flat under the upstream checkpoint's names ('.' -> '__'), reads and
writes upstream state dicts, keeps derived copies of weights (transposed, packed, concatenated) that must exist before
a graph capture and die when the parameters move or change, saves activations in `forward_train`, writes every `.grad`
in a hand-written `backward`, and hides behind ONE autograd node fed by a dummy `tick` tensor.  `FlatParamModule`
owns all of that; a model provides its list of names / shapes / initialisers, `forward_train`, `backward`, and where
its checkpoints need them the hooks `_extra_state` / `_tolerated_on_load`, `_CACHES` and `_CAPTURE_MSG`.

A model with train-mode dropout (the counter generator of csrc/dropout_rng.h) also keeps its `[seed, step]` state here:
`_drop_state_on` creates it at the first train-mode forward, `dropout_state` / `set_dropout_state` read and continue
it, `.to()` moves it.  It is no parameter and no buffer (absent from the state dict); a model whose probabilities are
all 0 never calls `_drop_state_on` and allocates nothing.  Hooks: `_drop_anchor` (the parameter whose device the state
follows) and `_DROP_CAPTURE_MSG`.
"""
import torch
from torch import nn

from . import ops


class FlatParamModule(nn.Module):
    _CACHES = ()  # names of the dicts of derived weight copies; `_drop_copies` empties them
    _CAPTURE_MSG = "derived weight copies must exist before a graph capture (run one eager step first)"
    _DROP_CAPTURE_MSG = "the dropout state must exist before a graph capture (run one eager step first)"
    _drop_state = None  # i64 [seed, step] on the device: not a parameter, not in the state dict

    def _register_flat(self, params):
        """params: ordered {upstream name: tensor | Parameter}; registration order = `named_parameters()` order."""
        self._names = list(params)
        for k, v in params.items():
            self.register_parameter(k.replace(".", "__"), v if isinstance(v, nn.Parameter) else nn.Parameter(v))
        for c in self._CACHES:
            setattr(self, c, {})
        self._wt_epoch = 0  # bumped whenever the copies are dropped (captured decode graphs go stale)
        self._saved = None

    def P(self, name):
        return getattr(self, name.replace(".", "__"))

    def _grad(self, name):
        p = self.P(name)
        if p.grad is None:
            p.grad = torch.empty_like(p)
        return p.grad

    # ---- upstream-compatible state dict ------------------------------------------------------------
    def _extra_state(self, prefix, keep_vars):
        """Keys the upstream state dict carries besides the parameters: {prefix + key: tensor}, in order."""
        return {}

    def _tolerated_on_load(self, key):
        """True for a foreign key (prefix stripped) that upstream checkpoints carry and this module ignores."""
        return False

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        for k in self._names:
            v = self.P(k)
            destination[prefix + k] = v if keep_vars else v.detach()
        destination.update(self._extra_state(prefix, keep_vars))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        mine = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        with torch.no_grad():
            for k in self._names:
                if k not in mine:
                    missing_keys.append(prefix + k)
                    continue
                src = torch.as_tensor(mine[k])
                if src.shape != self.P(k).shape:
                    error_msgs.append(f"size mismatch for {prefix + k}: {tuple(src.shape)} vs "
                                      f"{tuple(self.P(k).shape)}")
                else:
                    self.P(k).copy_(src)
        names = set(self._names)
        unexpected_keys.extend(prefix + k for k in mine if k not in names and not self._tolerated_on_load(k))
        self._drop_copies()

    # ---- derived copies of weights -------------------------------------------------------------------
    def _copy(self, cache, key, ref, make):
        """cache[key], built by `make()` when absent or on another device than `ref` (never during a capture)."""
        t = cache.get(key)
        if t is None or (t[0] if isinstance(t, tuple) else t).device != ref.device:
            if torch.cuda.is_current_stream_capturing():
                raise ops._lib.VsError(self._CAPTURE_MSG)
            t = cache[key] = make()
        return t

    def _drop_copies(self):
        for c in self._CACHES:
            getattr(self, c).clear()
        self._wt_epoch += 1

    def _apply(self, fn, *args, **kwargs):
        self._drop_copies()  # device / dtype moves replace the parameters' storage
        out = super()._apply(fn, *args, **kwargs)
        if self._drop_state is not None:  # the state moves with .to(); it stays int64 under a dtype cast
            self._drop_state = self._drop_state.to(self._drop_anchor().device)
        return out

    # ---- dropout state -------------------------------------------------------------------------------
    def _drop_anchor(self):
        """The parameter whose device the dropout state follows."""
        return self.P(self._names[0])

    @staticmethod
    def _site(snap, site, params):
        """The `drop` operand of one dropout site: (snap, site, thr, scale), None when its probability is 0."""
        return None if params is None else (snap, site) + params

    def _drop_state_on(self, device):
        """The persistent [seed, step] buffer on `device`; the seed is drawn from torch's default CPU generator at the
        first train-mode forward (so `torch.manual_seed` governs it)."""
        st = self._drop_state
        if st is None or st.device != device:
            if torch.cuda.is_current_stream_capturing():
                raise ops._lib.VsError(self._DROP_CAPTURE_MSG)
            if st is None:
                seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64))
                st = torch.tensor([seed, 0], dtype=torch.int64)
            st = self._drop_state = st.to(device)
        return st

    def dropout_state(self):
        """(seed, step) of the next train-mode forward, or None before the first one."""
        if self._drop_state is None:
            return None
        seed, step = self._drop_state.tolist()
        return seed, step

    def set_dropout_state(self, state):
        """Continue from `(seed, step)` (what `dropout_state()` returned).  Written in place when the buffer exists:
        captured training steps keep reading the same memory."""
        new = torch.tensor([int(state[0]), int(state[1])], dtype=torch.int64)
        if self._drop_state is None:
            self._drop_state = new.to(self._drop_anchor().device)
        else:
            self._drop_state.copy_(new)

    # ---- backward of a dense layer ---------------------------------------------------------------------
    def _linear_bwd(self, name, x, dy, bias=True, need_dx=True, conv1d=False, bf16=False, direct=False):
        """y = x W^T + b with W [out, in]: dW = dy^T x, db = colsum(dy), dx = dy W.  conv1d: huggingface's Conv1D,
        y = x W + b with W [in, out]: dW = x^T dy, and the parameter itself is the K-contiguous operand of dx.  bf16: both
        GEMMs take bf16 operands (ops.gemm_nt); the bias gradient stays an fp32 column sum.  direct: bf16 operands
        through the K-strided forms of ops.gemm_bf16, which read dy, x and W where they lie: no transposed copy."""
        w = self.P(name + ".weight")
        a, b = (x, dy) if conv1d else (dy, x)
        if direct:
            ops.gemm_bf16(a, b, out=self._grad(name + ".weight"), a_t=True, b_t=True)
        else:
            ops.gemm_nt(ops.transpose_f32(a), ops.transpose_f32(b), out=self._grad(name + ".weight"), bf16=bf16)
        if bias:
            ops.colsum_f32(dy, out=self._grad(name + ".bias"))
        if not need_dx:
            return None
        if direct:
            return ops.gemm_bf16(dy, w, b_t=not conv1d)
        return ops.gemm_nt(dy, w if conv1d else ops.transpose_f32(w), bf16=bf16)

    # ---- hand-over of the saved activations ------------------------------------------------------------
    def take_train_state(self):
        """The activations `forward_train` saved for `backward`, detached from the module (the autograd node keeps
        them: several forwards may precede a backward)."""
        st, self._saved = self._saved, None
        return st

    def put_train_state(self, st):
        self._saved = st


class FlatTrainFn(torch.autograd.Function):
    """`apply(model, *inputs, tick)`: the whole model as one autograd node.  `model.forward_train(*inputs)` returns one
    tensor or a tuple whose members may be None (those are dropped); `model.backward(*grads)` gets None for an absent
    or unused output, writes the parameters' `.grad` and returns the gradients of the inputs that require one, in
    their order (a tensor, a tuple or None)."""

    @staticmethod
    def forward(ctx, model, *args):
        inputs = args[:-1]  # the last one is the tick that makes autograd call backward
        ctx.model, ctx.n_in = model, len(inputs)
        ctx.set_materialize_grads(False)  # an output nobody used arrives as None, not as a tensor of zeros
        ctx.diff = [i for i, x in enumerate(inputs) if isinstance(x, torch.Tensor) and x.requires_grad]
        outs = model.forward_train(*[x.detach() if i in ctx.diff else x for i, x in enumerate(inputs)])
        # the saved activations of THIS forward travel with the node: a second forward before the backward
        # (two losses, gradient accumulation) must not replace them
        ctx.saved_state = model.take_train_state()
        if isinstance(outs, torch.Tensor):
            ctx.present = None
            return outs
        ctx.present = [o is not None for o in outs]
        return tuple(o for o in outs if o is not None)

    @staticmethod
    def backward(ctx, *grads):
        if ctx.present is not None:
            it = iter(grads)
            grads = [next(it) if present else None for present in ctx.present]
        ctx.model.put_train_state(ctx.saved_state)
        din = ctx.model.backward(*[None if g is None else g.contiguous() for g in grads])
        out = [None] * (ctx.n_in + 2)
        if din is not None:
            for i, g in zip(ctx.diff, din if isinstance(din, tuple) else (din,)):
                out[1 + i] = g
        return tuple(out)
