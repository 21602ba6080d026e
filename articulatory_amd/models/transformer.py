"""``Transformer`` — the feature-to-feature encoder (EMA -> mel and the like) behind the reference's ``generator_type`` plugin surface.

Drop-in for ``articulatory.models.Transformer`` (reference articulatory/models/transformer.py:21-105): same class name,
constructor keywords and defaults, the same state_dict keys, shapes and order — ``conv_blocks.N.{conv1,bn1,conv2,bn2,residual_path,res_norm}.*``
(the batch norms' buffers included), ``w_raw_in.*``, ``transformer.layers.N.self_attn.{w_q,w_k,w_v,w_o}``,
``...self_attn.relative_positional.embeddings``, ``linear1/2``, ``norm1/2``, ``w_out.*`` — and the same ``forward`` / ``inference`` /
``register_stats`` / ``remove_weight_norm``.  The modules below only HOLD parameters; the arithmetic runs in ``libhificar.so``
(``hificar_xfmr_*`` of include/hificar.h): no PyTorch-operator implementation, no CPU fallback.

In ``train()`` mode the forward is the reference's training-mode forward — the ResBlocks' ``BatchNorm1d`` on batch statistics with the
running-statistics update, ``Dropout(p)`` on the attention probabilities, behind both sub-blocks of every encoder layer and on the
feed-forward's hidden rows — under autograd: ``_TransformerFunction`` keeps a tape in ``hificar_xfmr_forward_train`` and routes
``hificar_xfmr_backward``'s gradients to every parameter (and to the input when it requires grad).  Dropout masks come from the package's
own counter-based generator (``set_dropout_seed``; numpy restatement: ``utils.synth.xfmr_dropout_mask``).

One deliberate difference: the reference pads its relative-position tables under ``torch.no_grad()`` (pytorch_layers.py:331-344), which cuts
them out of the graph — ``embeddings.grad`` stays None there and its optimizer never moves them from their initial values.  This package
computes the table's gradient (``train_relative_positions = True``, the default); set the attribute to False to train exactly what the
reference trains (the tables then get no gradient).

``forward_padded(x, lengths)`` trains on whole utterances of unequal lengths (this package's definition, the reference never masks):
``hificar_xfmr_forward_train_ragged`` through the same autograd node; the padded frames take no part in batch statistics, attention or
gradients.  ``forward_padded(x, lengths, packed=True)`` is the same step with no GEMM rows for the padding
(``hificar_xfmr_forward_train_packed`` / ``hificar_xfmr_backward_packed``): the same masks and definitions, results equal to rounding.

``precision="bf16x3"`` (opt-in; ``"f32"``, the reference's IEEE fp32 products, is the default) runs every GEMM of the eval-mode forward
in the conv engine's bf16x3 kernels (x w ~ hi hi + hi lo + lo hi on bf16 MFMAs, fp32 accumulation); attention, LayerNorm, bias and residual
additions and the residual stream stay fp32.  Inference only: a train()-mode forward of a bf16x3 model is refused.  Unlike
``HiFiGANGenerator`` the constructor does not read ``$HIFICAR_PRECISION``: the arithmetic of this model is chosen by keyword only.

``precision="bf16x3a"`` (opt-in, this model only) is ``"bf16x3"`` with the attention's three products — Q K^T, the relative-position product
Q E^T and P V — as hi hi + hi lo + lo hi on bf16 MFMAs as well, in a kernel of its own (``xfmr_attn16_kernel``) that reads q | k | v as split
rows and position tables split when the handle is built; the softmax itself, LayerNorm and the additions stay fp32.  Every bf16x3 rule holds:
inference only, keyword or ``set_precision`` only, kept by copies and ``load_state_dict``, not part of the ``state_dict``.  The generators
refuse the value.

``train_precision="bf16x3"`` (opt-in, keyword or ``set_train_precision``; ``"f32"`` is the default and unchanged) is the training step's
own switch, on a ``precision="f32"`` model: every forward GEMM of ``forward`` / ``forward_padded`` (packed or not) in train() mode and every
data gradient runs in the bf16x3 kernels, on weight fragments packed on the device after every optimizer step; weight and bias gradients,
the attention, the norms, dropout (the same masks) and the tape stay fp32, and so does the eval-mode forward.
``train_precision="bf16x3w"`` is that step with, in addition, the weight gradients of the one-tap layers at least 128 x 128 wide (``w_raw_in``,
q | k | v, ``w_o``, ``linear1``, ``linear2``) as G^T A ~ hi^T hi + hi^T lo + lo^T hi on bf16 MFMAs, and their bias gradients as the fp32 sum of
hi + lo; the k = 3 ResBlock convs, ``residual_path`` and ``w_out`` keep exact fp32 weight gradients.  ``precision="bf16x3w"`` is a ValueError.
``train_precision="bf16x3wa"`` is the bf16x3w step with, in addition, the training attention's query-tiled kernels on bf16 MFMAs: the forward
(Q K^T, the relative-position product, P V) and the backward's recomputed S, dO V^T and both parts of dQ, as hi hi + hi lo + lo hi with fp32
accumulation; the softmax statistics, dropout (the same masks), dS itself, dK, dV and the tables' gradient stay fp32, and so does the tape.
``precision="bf16x3wa"`` is a ValueError.
``train_precision="bf16x3wac"`` is the bf16x3wa step with, in addition, the weight and bias gradients of the wide k = 3 ResBlock convs
(``conv_blocks.{1,2}.conv1``, ``conv_blocks.{0,1,2}.conv2``, and ``conv_blocks.0.conv1`` where ``in_channels`` pads to 128 .. 1024 columns) on
bf16 MFMAs: each as a one-tap G^T A3 whose columns k cin + c hold frame t + k - 1 of channel c, zero outside the frame's own sequence.
``conv_blocks.0.conv1`` at other widths, ``residual_path`` and ``w_out`` keep exact fp32 weight gradients.  ``precision="bf16x3wac"`` is a
ValueError.
``train_precision="bf16x3wack"`` is the bf16x3wac step with, in addition, the attention's key-tiled backward on bf16 MFMAs: dK = dS^T Q / sqrt(d),
dV = Pd^T dO and the first stage of the tables' gradient dE[h][r] = sum dS[., r] Q as hi hi + hi lo + lo hi with fp32 accumulation, from the
same banded fp32 dS and Pd (dS, Pd and dQ themselves, the forward, the masks and the tape are bf16x3wac's bit for bit; no workspace of its
own).  ``precision="bf16x3wack"`` is a ValueError.
Not built: a k = 3 weight-gradient kernel that forms the three taps from one staged chunk, a key-major or pre-split copy of the dS / Pd bands.

Not built, refused with ``NotImplementedError``: ``extra_art=True`` and ``num_ph`` (phoneme input).  ``forward(lengths=...)`` in train() mode
is refused too (ragged training is asked for by name: ``forward_padded``).  The ``use_ar`` / ``ar_*`` / ``use_tanh`` / ``ph_emb_size``
keywords are accepted and unused, as in the reference.
``lengths=`` in eval mode is this package's addition: a ragged batch in which every utterance's result is that of running it alone.
"""

import ctypes
import logging
import math

import numpy as np
import torch

from .. import _native
from .bigru import _BatchNormParams, _LinearParams


class _Conv1dParams(torch.nn.Module):
    def __init__(self, cin, cout, k):
        super().__init__()
        b = 1.0 / math.sqrt(cin * k)  # torch.nn.Conv1d.reset_parameters
        self.weight = torch.nn.Parameter(torch.empty(cout, cin, k).uniform_(-b, b))
        self.bias = torch.nn.Parameter(torch.empty(cout).uniform_(-b, b))


class _ResBlockParams(torch.nn.Module):
    """ResBlock(num_ins, num_outs) (pytorch_layers.py:94-112), in its registration order."""

    def __init__(self, num_ins, num_outs):
        super().__init__()
        self.conv1 = _Conv1dParams(num_ins, num_outs, 3)
        self.bn1 = _BatchNormParams(num_outs)
        self.conv2 = _Conv1dParams(num_outs, num_outs, 3)
        self.bn2 = _BatchNormParams(num_outs)
        if num_ins != num_outs:
            self.residual_path = _Conv1dParams(num_ins, num_outs, 1)
            self.res_norm = _BatchNormParams(num_outs)


class _RelPosParams(torch.nn.Module):
    def __init__(self, max_relative_pos, num_heads, dim):
        super().__init__()
        self.embeddings = torch.nn.Parameter(torch.empty(num_heads, 2 * max_relative_pos - 1, dim, 1).normal_(0.0, dim ** -0.5))


class _AttentionParams(torch.nn.Module):
    """MultiHeadAttention(d_model, n_head, relative_positional=True) (pytorch_layers.py:180-203)."""

    def __init__(self, d_model, n_head, distance):
        super().__init__()
        d = d_model // n_head
        for name, shape in (("w_q", (n_head, d_model, d)), ("w_k", (n_head, d_model, d)), ("w_v", (n_head, d_model, d)), ("w_o", (n_head, d, d_model))):
            setattr(self, name, torch.nn.Parameter(torch.nn.init.xavier_normal_(torch.empty(shape))))
        self.relative_positional = _RelPosParams(distance, n_head, d)


class _LayerNormParams(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(n))
        self.bias = torch.nn.Parameter(torch.zeros(n))


class _EncoderLayerParams(torch.nn.Module):
    """TransformerEncoderLayer (pytorch_layers.py:147-160), in its registration order."""

    def __init__(self, d_model, n_head, dim_feedforward, distance):
        super().__init__()
        self.self_attn = _AttentionParams(d_model, n_head, distance)
        self.linear1 = _LinearParams(d_model, dim_feedforward)
        self.linear2 = _LinearParams(dim_feedforward, d_model)
        self.norm1 = _LayerNormParams(d_model)
        self.norm2 = _LayerNormParams(d_model)


class _EncoderParams(torch.nn.Module):
    """torch.nn.TransformerEncoder's only parameter-bearing attribute: ``layers``."""

    def __init__(self, layers):
        super().__init__()
        self.layers = torch.nn.ModuleList(layers)


def _grad_layout(module):
    """[(state_dict key, offset, numel)] of the native gradient buffer (hificar_xfmr_grad_info), cached per handle."""
    cached = module.__dict__.get("_grad_info")
    if cached is not None and cached[0] == id(module._handle):
        return cached[1]
    lib, handle = module._lib, module._handle
    out = []
    name = ctypes.create_string_buffer(96)
    off, num = ctypes.c_int64(), ctypes.c_int64()
    for i in range(lib.hificar_xfmr_grad_count(handle)):
        _native.check(lib.hificar_xfmr_grad_info(handle, i, name, ctypes.byref(off), ctypes.byref(num)), "hificar_xfmr_grad_info")
        out.append((name.value.decode(), off.value, num.value))
    module.__dict__["_grad_info"] = (id(module._handle), out)
    return out


class _TransformerFunction(torch.autograd.Function):
    """Autograd node of the native Transformer in train() mode: forward = hificar_xfmr_forward_train (or, with ``module._lens`` set by
    ``forward_padded``, hificar_xfmr_forward_train_ragged: the lengths are read here, at forward time, and live on in the tape), backward =
    hificar_xfmr_backward (``module._packed``: the packed pair of entry points).  Inputs after (module, x, p, seed, offset, names) are the
    module's parameters in ``names`` order.  Returns (out, batch statistics (number of batch norms, 2, hidden_dim): mean | biased variance); the statistics carry no gradient."""

    @staticmethod
    def forward(ctx, module, x, p, seed, offset, names, *params):
        out, stats, tape, toff = module._run_forward_train(x, p, seed, offset, keep_tape=True, lens=module._lens, packed=module._packed)
        B, _, T = x.shape
        ctx.module, ctx.names, ctx.tape, ctx.toff, ctx.BT = module, names, tape, toff, (B, T)
        ctx.packed_lens = module._lens[0] if module._packed else None  # the host lengths: hificar_xfmr_backward_packed checks them
        ctx.save_for_backward(*params)  # torch's own version check covers an in-place edit that bumps Parameter._version ...
        ctx.steps_seen = module._steps_seen  # ... and this one a fused optimizer step, which does not
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    def backward(ctx, dout, _dstats=None):
        module = ctx.module
        lib, handle = module._lib, module._handle
        B, T = ctx.BT
        params = ctx.saved_tensors
        if handle is None or ctx.steps_seen != module._steps_seen:
            raise RuntimeError("a Transformer parameter was modified between forward and backward (the backward pass reads the weights the "
                               "forward used)")
        dev = ctx.tape.device
        dout = dout.to(torch.float32).contiguous()
        dx = torch.empty((B, module._params["in_channels"], T), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            grads = torch.empty(int(lib.hificar_xfmr_grad_floats(handle)), dtype=torch.float32, device=dev)
            tail = (ctx.tape.data_ptr() + ctx.toff, ctx.tape.numel() - ctx.toff, grads.data_ptr(), dx.data_ptr() if dx is not None else None)
            if ctx.packed_lens is None:
                ws_ptr, ws_bytes = module._train_workspace(B, T)
                rc = lib.hificar_xfmr_backward(handle, dout.data_ptr(), B, T, *tail, ws_ptr, ws_bytes, stream)
            else:
                ws_ptr, ws_bytes = module._train_workspace(B, T, module._packed_rows(ctx.packed_lens, B, T))
                rc = lib.hificar_xfmr_backward_packed(handle, dout.data_ptr(), ctx.packed_lens.data_ptr(), B, T, *tail, ws_ptr, ws_bytes, stream)
        _native.check(rc, "hificar_xfmr_backward" if ctx.packed_lens is None else "hificar_xfmr_backward_packed")
        views = {name: grads[off:off + num] for name, off, num in _grad_layout(module)}
        skip = () if module.train_relative_positions else ("relative_positional.embeddings",)
        gw = tuple(views[n].view(t.shape) if need and not n.endswith(skip or ("\0",)) else None
                   for n, t, need in zip(ctx.names, params, ctx.needs_input_grad[6:]))
        ctx.tape = None
        return (None, dx, None, None, None, None, *gw)


class _PrecisionKeyword(type):
    """``Transformer(..., precision=None)``: this package's one constructor keyword beyond the reference's, taken by the class call so that
    ``Transformer.__init__`` keeps the reference's signature, keyword for keyword (drop-in code inspects it).  None: "f32" —
    ``$HIFICAR_PRECISION`` is deliberately not consulted (see the module's docstring); anything but "f32" / "bf16x3" / "bf16x3a": ValueError."""

    def __call__(cls, *args, precision=None, train_precision=None, **kwargs):
        if precision is None:
            precision = "f32"
        if precision not in _native.XFMR_PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_native.XFMR_PRECISIONS)}")
        if train_precision is None:
            train_precision = "f32"
        if not isinstance(train_precision, str) or train_precision not in _native.XFMR_TRAIN_PRECISIONS_K:
            raise ValueError(f"train_precision must be one of {sorted(_native.XFMR_TRAIN_PRECISIONS_K)}")
        if precision != "f32" and train_precision != "f32":
            raise ValueError(f"train_precision='{train_precision}' needs precision='f32': a precision='{precision}' model is inference-only")
        self = super().__call__(*args, **kwargs)
        self.precision = precision
        self.train_precision = train_precision
        return self


class Transformer(torch.nn.Module, metaclass=_PrecisionKeyword):
    """Three ResBlocks -> Linear -> ``elayers`` post-LayerNorm encoder layers (8 heads, learned relative positions, 3072-wide feed-forward)
    -> Linear; MI355X-native, eval and train().  ``precision="bf16x3"`` (keyword only): see the module's docstring and ``set_precision``."""

    def __init__(self, in_channels=8, out_channels=80, elayers=6, hidden_dim=768, dropout=.2, extra_art=False,
                 use_ar=False, ar_input=512, ar_hidden=256, ar_output=128, use_tanh=False,
                 num_ph=None, ph_emb_size=8, layer_type='default'):
        super().__init__()
        self.precision = "f32"  # (Transformer(..., precision=...): _PrecisionKeyword)
        self.train_precision = "f32"  # (Transformer(..., train_precision=...): the same)
        if extra_art:
            raise NotImplementedError("Transformer(extra_art=True) is not built (its kernel-size-2 input conv shortens the sequence by a frame)")
        if num_ph is not None:
            raise NotImplementedError("Transformer(num_ph=...) is not built (phoneme input: the ph2a / ph2m decode modes are not built either)")
        if layer_type != 'default':
            raise NotImplementedError(f"layer_type {layer_type} not supported")  # (the reference logs this and exits, transformer.py:44-46)
        self._params = dict(in_channels=in_channels, out_channels=out_channels, elayers=elayers, hidden_dim=hidden_dim, dropout=dropout)
        _native.check_xfmr_params(self._params)  # libhificar's own limits: fail here, before any device work
        self.conv_blocks = torch.nn.Sequential(_ResBlockParams(in_channels, hidden_dim), _ResBlockParams(hidden_dim, hidden_dim),
                                               _ResBlockParams(hidden_dim, hidden_dim))
        self.w_raw_in = _LinearParams(hidden_dim, hidden_dim)
        self.transformer = _EncoderParams([_EncoderLayerParams(hidden_dim, _native.XFMR_HEADS, _native.XFMR_FF, _native.XFMR_REL)
                                           for _ in range(elayers)])
        self.w_out = _LinearParams(hidden_dim, out_channels)
        self.in_emb_mat = None
        self._handle = None
        self._lib = None
        self._workspace_buf = None
        self._sig = None
        self._train_ws_buf = None
        self._on_device = False  # the handle's weights are refreshed from device tensors (set once a training forward ran on it)
        self._dirty = False      # an optimizer stepped since the last hand-over (fused optimizers do not bump Parameter._version)
        self._steps_seen = 0     # optimizer steps noticed so far
        self._calls = 0          # training forwards so far: the dropout generator's offset
        self._lens = None        # the lengths of the ragged training forward under way (forward_padded)
        self._packed = False     # ... and whether it is the packed form
        self._last_stats = None
        self.train_relative_positions = True  # False: the tables get no gradient, as in the reference (see the module's docstring)
        # drawn from torch's generator (after the parameters): torch.manual_seed makes a training run repeatable
        self._dropout_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        from ..utils.optim_hook import watch

        watch(self)  # fused optimizers do not bump Parameter._version: every optimizer.step() over these parameters marks them stale

    def set_precision(self, precision):
        """Arithmetic of the following eval-mode forwards: "f32", "bf16x3" or "bf16x3a".  The native handle holds the weight fragments of one
        arithmetic only, so a change drops it: the next forward builds a new handle from the parameters' host copies
        (hificar_xfmr_set_precision between create and finalize).  A model that has just trained in fp32 can therefore be switched to
        bf16x3 for evaluation, at the cost of one trip of its weights through the host (and one more to switch back)."""
        if precision not in _native.XFMR_PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_native.XFMR_PRECISIONS)}")
        if precision != "f32" and self.train_precision != "f32":
            raise ValueError(f"precision='{precision}' is inference-only: set_train_precision('f32') first")
        if precision != self.precision:
            self.precision = precision
            self._invalidate()

    def set_train_precision(self, train_precision):
        """Arithmetic of the following train()-mode forwards and their backward passes: "f32" (the default) or "bf16x3" — every forward GEMM
        and every data gradient as x w ~ hi hi + hi lo + lo hi on bf16 MFMAs with fp32 accumulation; weight and bias gradients, attention,
        norms, dropout and the tape stay fp32 (hificar_xfmr_set_train_precision).  The eval-mode forward is exact fp32 either way.  The
        native handle is kept: its packs are rebuilt on the device.  A backward whose forward ran in the other arithmetic is refused
        (RuntimeError).  "bf16x3w": "bf16x3", and the weight and bias gradients of the one-tap layers at least 128 x 128 wide in the same
        arithmetic; "bf16x3wa": "bf16x3w", and the attention's query-tiled kernels on bf16 MFMAs; "bf16x3wac": "bf16x3wa", and the weight
        gradients of the wide k = 3 convs on bf16 MFMAs; "bf16x3wack": "bf16x3wac", and the attention's dK, dV and table gradients on bf16
        MFMAs (see the module's docstring).  Not with
        ``precision="bf16x3"`` (ValueError)."""
        if not isinstance(train_precision, str) or train_precision not in _native.XFMR_TRAIN_PRECISIONS_K:
            raise ValueError(f"train_precision must be one of {sorted(_native.XFMR_TRAIN_PRECISIONS_K)}")
        if train_precision != "f32" and self.precision != "f32":
            raise ValueError(f"train_precision='{train_precision}' needs precision='f32': a precision='{self.precision}' model is inference-only")
        if train_precision == self.train_precision:
            return
        self.train_precision = train_precision
        if self.__dict__.get("_handle") is not None:
            with torch.cuda.device(self._device()):
                _native.check(self._lib.hificar_xfmr_set_train_precision(self._handle, _native.XFMR_TRAIN_PRECISIONS_K[train_precision]),
                              "hificar_xfmr_set_train_precision")

    def _refuse_bf16x3_training(self):
        if self.precision != "f32":
            raise RuntimeError(f"training runs in the exact-fp32 arithmetic: this Transformer has precision='{self.precision}' "
                               "(set_precision('f32') before train()-mode forwards)")

    # ------------------------------------------------------------------ training surface
    def set_dropout_seed(self, seed, offset=0):
        """Seed of the dropout masks; the count of training forwards (the generator's offset) restarts at ``offset``."""
        self._dropout_seed = int(seed) & (2 ** 64 - 1)
        self._calls = int(offset)

    def invalidate_parameters(self):
        """The parameters changed in place without their version counters showing it (what ``utils.optim_hook`` calls after every
        ``optimizer.step()``): the next forward hands them to the native handle again."""
        self._dirty = True
        self._steps_seen += 1

    def _batch_norms(self):
        """The BatchNorm1d holders in registration order: the order of hificar_xfmr_forward_train's bn_batch_stats."""
        out = []
        for blk in self.conv_blocks:
            out += [blk.bn1, blk.bn2]
            if hasattr(blk, "res_norm"):
                out.append(blk.res_norm)
        return out

    # ------------------------------------------------------------------ reference surface
    def remove_weight_norm(self):
        """Nothing carries weight norm (transformer.py:97-98); articulatory_amd.bin.decode calls it on every model."""

    def register_stats(self, stats):
        """Register mean/scale buffers (transformer.py:79-95)."""
        assert stats.endswith(".h5") or stats.endswith(".npy")
        if stats.endswith(".h5"):
            from ..utils.hdf5 import read_hdf5

            mean = read_hdf5(stats, "mean").reshape(-1)
            scale = read_hdf5(stats, "scale").reshape(-1)
        else:
            arr = np.load(stats)
            mean = arr[0].reshape(-1)
            scale = arr[1].reshape(-1)
        self.register_buffer("mean", torch.from_numpy(np.asarray(mean)).float())
        self.register_buffer("scale", torch.from_numpy(np.asarray(scale)).float())
        logging.info("Successfully registered stats as buffer.")

    def inference(self, x, normalize_before=False):
        """(T, in_channels) -> (T, out_channels), transformer.py:100-105 statement for statement.  The reference takes ``normalize_before`` and
        never normalises for this class; asking for it is refused instead of ignored."""
        if normalize_before:
            raise NotImplementedError("Transformer.inference(normalize_before=True): the reference's Transformer.inference never normalises "
                                      "its input (transformer.py:100-105 ignores the flag); normalise the features before the call")
        if not isinstance(x, torch.Tensor):
            x = torch.tensor(x, dtype=torch.float).to(self._device())
        x = x.unsqueeze(0)
        if len(x.shape) == 3:
            x = x.permute(0, 2, 1)
        out = self.forward(x)
        return out.squeeze(0).transpose(1, 0)

    # ------------------------------------------------------------------ native handle
    def _device(self):
        return self.w_out.weight.device

    def native_state(self):
        """{reference state_dict key: fp32 CPU tensor} of what the C ABI consumes (every float tensor but the input statistics)."""
        out = {}
        for k, v in self.state_dict().items():
            if k in ("mean", "scale") or k.endswith("num_batches_tracked"):
                continue
            out[k] = v.detach().float().cpu().contiguous()
        return out

    def _signature(self):
        ts = list(self.parameters()) + [b for n, b in self.named_buffers() if n.endswith(("running_mean", "running_var"))]
        return tuple((t.data_ptr(), t._version) for t in ts)

    def _invalidate(self):
        h = self.__dict__.get("_handle")
        if h is not None and self._lib is not None:
            self._lib.hificar_xfmr_destroy(h)
        self._handle = None
        self._workspace_buf = None
        self._train_ws_buf = None
        self._sig = None
        self._on_device = False
        self._dirty = False

    def __del__(self):
        try:
            self._invalidate()
        except Exception:
            pass

    def __getstate__(self):  # copies and pickles never share a native handle
        state = self.__dict__.copy()
        for k in ("_handle", "_lib", "_workspace_buf", "_sig", "_train_ws_buf", "_last_stats", "_lens"):
            state[k] = None
        state["_on_device"] = state["_dirty"] = False
        state.pop("_grad_info", None)
        return state

    def __setstate__(self, state):
        state.setdefault("train_precision", "f32")  # (a pickle from before the keyword)
        super().__setstate__(state)
        from ..utils.optim_hook import watch

        watch(self)  # a copy trains with its own optimizer

    def load_state_dict(self, state_dict, strict=True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._invalidate()
        return out

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        self._invalidate()
        return out

    def refresh_native(self):
        """Re-upload the weights after an in-place parameter edit that the version counters do not show (``p.data.copy_``)."""
        self._invalidate()

    def _send_parameters(self):
        """Every float tensor of the state_dict from device memory into the handle (hificar_xfmr_set_parameters_device): nothing goes
        through the host.  The tensors are read on the current stream, in stream order with the optimizer step that wrote them."""
        names, held = [], []
        for k, v in self.state_dict(keep_vars=True).items():
            if k in ("mean", "scale") or k.endswith("num_batches_tracked"):
                continue
            names.append(k)
            held.append(v if (v.dtype == torch.float32 and v.is_contiguous()) else v.detach().to(torch.float32).contiguous())
        arr = (ctypes.c_char_p * len(names))(*[n.encode() for n in names])
        ptrs = (ctypes.c_void_p * len(held))(*[t.data_ptr() for t in held])
        with torch.cuda.device(self._device()):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            _native.check(self._lib.hificar_xfmr_set_parameters_device(self._handle, arr, ptrs, len(held), stream),
                          "hificar_xfmr_set_parameters_device")
        self._on_device = True
        self._dirty = False
        self._sig = self._signature()

    def _native_handle(self, train=False):
        if self._handle is not None and self._on_device:
            # a handle that has trained: its weights follow the parameters on the device (eval after training sees the updated weights and
            # running statistics without a trip through the host)
            if self._dirty or self._sig != self._signature():
                self._send_parameters()
            return self._handle
        if self._handle is not None and self._sig == self._signature() and not self._dirty:
            if train:
                self._send_parameters()
            return self._handle
        self._invalidate()
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("Transformer: parameters are on %s; the forward only exists as HIP kernels (move the model to a MI355X with "
                               ".to('cuda')). There is no CPU fallback." % (dev,))
        lib = _native.load_library()
        self._lib = lib
        handle = ctypes.c_void_p()
        with torch.cuda.device(dev):
            cfg = _native.make_xfmr_config(self._params)
            _native.check(lib.hificar_xfmr_create(ctypes.byref(cfg), ctypes.byref(handle)), "hificar_xfmr_create")
            try:
                for name, t in self.native_state().items():
                    shape = (ctypes.c_int64 * t.dim())(*t.shape)
                    _native.check(lib.hificar_xfmr_set_weight(handle, name.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim()),
                                  "hificar_xfmr_set_weight")
                _native.check(lib.hificar_xfmr_set_precision(handle, _native.XFMR_PRECISIONS[self.precision]), "hificar_xfmr_set_precision")
                _native.check(lib.hificar_xfmr_finalize(handle), "hificar_xfmr_finalize")
                if self.precision == "f32":  # (a bf16x3 inference handle has no training arithmetic to choose)
                    _native.check(lib.hificar_xfmr_set_train_precision(handle, _native.XFMR_TRAIN_PRECISIONS_K[self.train_precision]),
                                  "hificar_xfmr_set_train_precision")
            except Exception:
                lib.hificar_xfmr_destroy(handle)
                raise
        self._handle = handle
        self._sig = self._signature()
        if train:
            self._send_parameters()
        return handle

    def _packed_rows(self, host_lens, B, T):
        """Mp of a packed batch (hificar_xfmr_packed_rows), from the host lengths."""
        mp = int(self._lib.hificar_xfmr_packed_rows(B, T, host_lens.data_ptr()))
        if mp <= 0:
            raise RuntimeError(f"Transformer.forward_padded(packed=True): a batch of {B} x {T} with {int(host_lens.sum())} frames cannot be packed "
                               "(at least two frames; packed rows * 3072 < 2^31)")
        return mp

    def _train_workspace(self, B, T, packed_rows=None):
        """One grow-only scratch buffer shared by the training forward and the backward pass (hificar_xfmr_train_workspace_bytes, or, for a
        packed step of ``packed_rows`` rows, hificar_xfmr_train_workspace_bytes_packed)."""
        if packed_rows is None:
            n = self._lib.hificar_xfmr_train_workspace_bytes(self._handle, B, T) + 256
        else:
            n = self._lib.hificar_xfmr_train_workspace_bytes_packed(self._handle, B, packed_rows) + 256
        ws = self._train_ws_buf
        if ws is None or ws.numel() < n:
            ws = torch.empty(int(n * 1.25) if ws is not None else n, dtype=torch.uint8, device=self._device())
            self._train_ws_buf = ws
        off = (-ws.data_ptr()) % 256
        return ws.data_ptr() + off, ws.numel() - off

    def _run_forward_train(self, x, p, seed, offset, keep_tape, lens=None, packed=False):
        """hificar_xfmr_forward_train (lens = (host, device) int32 lengths: hificar_xfmr_forward_train_ragged, or, packed,
        hificar_xfmr_forward_train_packed) on the current stream: (out, batch statistics, tape or None, the tape's alignment offset)."""
        lib, handle = self._lib, self._handle
        B, _, T = x.shape
        dev = x.device
        mp = self._packed_rows(lens[0], B, T) if packed else None
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            tape, toff = None, 0
            if keep_tape:
                nbytes = lib.hificar_xfmr_tape_bytes_packed(handle, B, mp) if packed else lib.hificar_xfmr_tape_bytes(handle, B, T)
                tape = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
                toff = (-tape.data_ptr()) % 256
            out = torch.empty((B, self._params["out_channels"], T), dtype=torch.float32, device=dev)
            stats = torch.empty((len(self._batch_norms()), 2, self._params["hidden_dim"]), dtype=torch.float32, device=dev)
            ws_ptr, ws_bytes = self._train_workspace(B, T, mp)
            tail = (B, T, float(p), seed, offset, tape.data_ptr() + toff if keep_tape else None, tape.numel() - toff if keep_tape else 0,
                    ws_ptr, ws_bytes, stream)
            what = "hificar_xfmr_forward_train" if lens is None else "hificar_xfmr_forward_train_packed" if packed else "hificar_xfmr_forward_train_ragged"
            if lens is None:
                rc = lib.hificar_xfmr_forward_train(handle, x.data_ptr(), out.data_ptr(), stats.data_ptr(), *tail)
            else:
                rc = getattr(lib, what)(handle, x.data_ptr(), lens[1].data_ptr(), lens[0].data_ptr(), out.data_ptr(), stats.data_ptr(), *tail)
        _native.check(rc, what)
        return out, stats, tape, toff

    def _workspace(self, B, T, factor=None):
        """One grow-only scratch buffer per model (hificar_xfmr_workspace_bytes; ``factor``: T low-rate frames,
        hificar_xfmr_workspace_bytes_lowrate)."""
        if factor is None:
            n = self._lib.hificar_xfmr_workspace_bytes(self._handle, B, T) + 256
        else:
            n = self._lib.hificar_xfmr_workspace_bytes_lowrate(self._handle, B, T, factor)
            if n == 0:
                raise RuntimeError(f"Transformer.forward_lowrate: B={B}, Tl={T}, interp_factor={factor} out of range (B factor Tl 3072 < 2^31)")
            n += 256
        ws = self._workspace_buf
        if ws is None or ws.numel() < n:
            # work already enqueued on the old buffer keeps it alive through the caching allocator's stream ordering
            ws = torch.empty(int(n * 1.25) if ws is not None else n, dtype=torch.uint8, device=self._device())
            self._workspace_buf = ws
        off = (-ws.data_ptr()) % 256
        return ws.data_ptr() + off, ws.numel() - off

    def engine(self):
        """The engine handle for ``hificar_profile_begin`` / ``hificar_profile_end`` (per-kernel device times; tools/transformer_bench.py)."""
        handle = self._native_handle()  # first: it is what loads self._lib
        return ctypes.c_void_p(self._lib.hificar_xfmr_engine(handle))

    def debug_tap(self, name, dst=None):
        """Test aid (hificar_xfmr_debug_tap): the following forwards copy intermediate ``name`` — "conv_blocks", "w_raw_in", "layers.N.norm1",
        "layers.N" — as rows (B, T, hidden_dim) into the float32 CUDA tensor ``dst``; ``dst=None`` forgets it, ``name=None`` all of them.  A
        bf16x3 model refuses "conv_blocks" (those rows exist as split bf16 rows only).  A train()-mode forward serves its ReLU outputs: "conv_blocks.N.relu1", "conv_blocks.N.relu2" and "layers.N.hidden" (B, T, 3072)."""
        handle = self._native_handle()
        _native.check(self._lib.hificar_xfmr_debug_tap(handle, name.encode() if name is not None else None, dst.data_ptr() if dst is not None else None,
                                                       dst.numel() if dst is not None else 0), "hificar_xfmr_debug_tap")

    # ------------------------------------------------------------------ forward
    def forward(self, x, spk_id=None, ar=None, ph=None, lengths=None):
        """x: (B, in_channels, T) -> (B, out_channels, T)  (transformer.py:55-77, eval mode).  ``spk_id``, ``ar`` and ``ph`` are accepted and
        ignored, as in the reference.  ``lengths`` (B frame counts): a ragged batch — utterance b is computed as if it were alone with
        lengths[b] frames (the convs see zero padding at its own end, its keys stop at its length), out[b, :, lengths[b]:] is zero, and
        what x holds past a length is never read."""
        if self.training:
            self._refuse_bf16x3_training()  # (before any device check)
            return self._forward_train(x, lengths)
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise RuntimeError("Transformer.forward needs a CUDA/HIP tensor; there is no CPU fallback")
        if x.dim() != 3 or x.shape[1] != self._params["in_channels"]:
            raise RuntimeError(f"Transformer.forward: expected (B, {self._params['in_channels']}, T), got {tuple(x.shape)}")
        handle = self._native_handle()
        if x.device != self._device():
            raise RuntimeError(f"Transformer.forward: input on {x.device}, parameters on {self._device()}")
        c = x.detach().to(torch.float32).contiguous()
        B, _, T = c.shape
        if B < 1 or T < 1:
            raise RuntimeError(f"Transformer.forward: empty input {tuple(c.shape)}")
        lens = (None, None)
        keep = None
        if lengths is not None:
            keep = self._check_lengths(lengths, B, T, c.device)
            lens = (keep[1].data_ptr(), keep[0].data_ptr())
        out = torch.empty((B, self._params["out_channels"], T), dtype=torch.float32, device=c.device)
        with torch.cuda.device(c.device):
            ws_ptr, ws_bytes = self._workspace(B, T)
            stream = torch.cuda.current_stream().cuda_stream
            rc = self._lib.hificar_xfmr_forward(handle, c.data_ptr(), lens[0], lens[1], out.data_ptr(), B, T, ws_ptr, ws_bytes,
                                                ctypes.c_void_p(stream))
        _native.check(rc, "hificar_xfmr_forward")
        return out

    def forward_lowrate(self, x, lengths=None, interp_factor=1, zscore=False):
        """The reference's speech-to-EMA front end and the forward behind it in one call (egs/ema/voc1/local/predict_ema.py:83-101), eval mode:
        x (B, in_channels, Tl) features as the speech model or the MFCC extraction delivers them -> (B, out_channels, interp_factor * Tl).
        ``interp_factor`` (an integer in 1 .. 16; the reference uses 4, or 2 for its hprc models): every utterance is stretched as
        ``F.interpolate(x_b[..., :l_b], size=interp_factor * l_b, mode='linear', align_corners=False)`` does, clamped at its own first and last
        frame.  ``zscore``: every utterance is first normalised by the mean and the population standard deviation of all its in_channels x l_b
        elements (``scipy.stats.zscore(feat, axis=None)``, predict_ema.py:32-35; a constant utterance gives NaN, as scipy does).  ``lengths``
        (B LOW-RATE frame counts): a ragged batch — an utterance's result is bitwise that of running it alone, the output is zero past
        interp_factor * lengths[b], and padded input frames are never read.  Neither the stretched nor the normalised input is ever
        materialised: the input rows are formed at the model's rate from the low-rate input, at any ``precision``.  ``interp_factor=1, zscore=False`` is ``forward(x, lengths=lengths)``."""
        f = _native.check_interp_factor(interp_factor)
        if self.training:
            raise NotImplementedError("Transformer.forward_lowrate: the low-rate front end is an inference path (call .eval(); training on "
                                      "low-rate inputs is not built)")
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise RuntimeError("Transformer.forward_lowrate needs a CUDA/HIP tensor; there is no CPU fallback")
        if x.dim() != 3 or x.shape[1] != self._params["in_channels"]:
            raise RuntimeError(f"Transformer.forward_lowrate: expected (B, {self._params['in_channels']}, Tl), got {tuple(x.shape)}")
        handle = self._native_handle()
        if x.device != self._device():
            raise RuntimeError(f"Transformer.forward_lowrate: input on {x.device}, parameters on {self._device()}")
        c = x.detach().to(torch.float32).contiguous()
        B, _, Tl = c.shape
        if B < 1 or Tl < 1:
            raise RuntimeError(f"Transformer.forward_lowrate: empty input {tuple(c.shape)}")
        lens = (None, None)
        keep = None
        if lengths is not None:
            keep = self._check_lengths(lengths, B, Tl, c.device)
            lens = (keep[1].data_ptr(), keep[0].data_ptr())
        out = torch.empty((B, self._params["out_channels"], f * Tl), dtype=torch.float32, device=c.device)
        with torch.cuda.device(c.device):
            ws_ptr, ws_bytes = self._workspace(B, Tl, factor=f)
            stream = torch.cuda.current_stream().cuda_stream
            rc = self._lib.hificar_xfmr_forward_lowrate(handle, c.data_ptr(), lens[0], lens[1], out.data_ptr(), B, Tl, f, 1 if zscore else 0, ws_ptr,
                                           ws_bytes, ctypes.c_void_p(stream))
        _native.check(rc, "hificar_xfmr_forward_lowrate")
        return out

    def forward_padded(self, x, lengths, packed=False):
        """A batch of whole utterances, zero-padded to (B, in_channels, T), with their frame counts ``lengths`` (B values in 0 .. T).
        eval(): ``forward(x, lengths=lengths)``.  train(): the training step on the ragged batch, under autograd — this package's
        definition, the reference never masks: the convs see zero padding at a sequence's own end, a query's keys lie below its sequence's
        own length, dropout masks are those of the padded tensors (they depend on T), every batch norm takes mean and biased variance over
        the M = sum(lengths) valid frames (running variance: M / (M - 1)), ``out[b, :, lengths[b]:]`` is exactly zero; backwards, the output
        gradient on padded frames is ignored whatever it holds, the input gradient is zero there, and every parameter gradient sums valid
        frames only.  With every length equal to T all results are bitwise those of ``forward``.  What ``x`` holds in padded frames is
        never used.
        ``packed=True`` (train() only; eval() ignores it): the same step, the same masks at the same seed, computed without GEMM rows for the
        padding (hificar_xfmr_forward_train_packed): the sums over rows run in another order, so results equal the unpacked step's to
        rounding, not bitwise."""
        if not self.training:
            return self.forward(x, lengths=lengths)
        self._refuse_bf16x3_training()
        if lengths is None:
            raise RuntimeError("Transformer.forward_padded needs lengths")
        return self._forward_train(x, lengths, padded=True, packed=bool(packed))

    def _forward_train(self, x, lengths, padded=False, packed=False):
        """train() mode (transformer.py:55-77 with every nn.Dropout active and the batch norms on batch statistics): with grad enabled the
        output is part of the autograd graph; without, the same arithmetic runs and its tape is dropped.  Every call — either way —
        advances the dropout generator's offset and updates every batch norm's running_mean / running_var / num_batches_tracked as
        torch.nn.BatchNorm1d does."""
        if lengths is not None and not padded:
            raise NotImplementedError("Transformer.forward(lengths=...) in train() mode is refused: ragged training uses masked batch "
                                      "statistics, this package's definition and not the reference's, so asking for it is explicit: call "
                                      "forward_padded(x, lengths) (or .eval() for ragged inference)")
        if padded and packed and isinstance(x, torch.Tensor) and x.dim() == 3:  # the lengths first: checking them needs no device
            self._check_lengths(lengths, x.shape[0], x.shape[2], torch.device("cpu"))
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise NotImplementedError("Transformer.forward in train() mode needs a CUDA/HIP tensor: the training path exists on the device "
                                      "only, as HIP kernels (there is no CPU fallback)")
        if x.dim() != 3 or x.shape[1] != self._params["in_channels"]:
            raise RuntimeError(f"Transformer.forward: expected (B, {self._params['in_channels']}, T), got {tuple(x.shape)}")
        B, _, T = x.shape
        if B < 1 or T < 1:
            raise RuntimeError(f"Transformer.forward: empty input {tuple(x.shape)}")
        n = B * T
        lens = None
        if padded:
            lens = self._check_lengths(lengths, B, T, x.device)
            n = int(lens[0].sum())
        if n < 2:  # torch.nn.functional.batch_norm's own refusal
            raise ValueError("Expected more than 1 value per channel when training, got input size "
                             f"{[B, self._params['hidden_dim'], T] if lens is None else [n, self._params['hidden_dim']]}")
        self._native_handle(train=True)
        if x.device != self._device():
            raise RuntimeError(f"Transformer.forward: input on {x.device}, parameters on {self._device()}")
        if padded and packed:
            self._packed_rows(lens[0], B, T)  # (a batch too large to pack is refused here, before a mask is drawn)
        c = x.to(torch.float32).contiguous()
        named = list(self.named_parameters())
        names, params = tuple(k for k, _ in named), [p for _, p in named]
        offset = self._calls
        self._calls += 1
        self._lens, self._packed = lens, packed and padded
        try:
            if torch.is_grad_enabled() and (c.requires_grad or any(p.requires_grad for p in params)):
                out, stats = _TransformerFunction.apply(self, c, self._params["dropout"], self._dropout_seed, offset, names, *params)
            else:  # no graph: the same arithmetic without a tape (tape = NULL)
                out, stats, _, _ = self._run_forward_train(c.detach(), self._params["dropout"], self._dropout_seed, offset, keep_tape=False, lens=lens,
                                                            packed=self._packed)
        finally:
            self._lens, self._packed = None, False
        self._last_stats = stats.detach()  # (number of batch norms, 2, hidden_dim): this batch's mean | biased variance, for inspection
        with torch.no_grad():  # torch.nn.BatchNorm1d: momentum 0.1, the running variance takes the UNBIASED batch variance (n: the valid frames)
            for j, bn in enumerate(self._batch_norms()):
                bn.running_mean.mul_(0.9).add_(stats[j, 0], alpha=0.1)
                bn.running_var.mul_(0.9).add_(stats[j, 1], alpha=0.1 * n / (n - 1))
                bn.num_batches_tracked += 1
        # (the running statistics only enter the eval path: its folds are refreshed when an eval forward next asks for the handle)
        return out

    @staticmethod
    def _check_lengths(lengths, B, T, device):
        """(host int32 tensor, its copy on ``device``) of B frame counts in 0 .. T."""
        host = (lengths.detach().to("cpu", torch.int32) if isinstance(lengths, torch.Tensor) else torch.as_tensor(lengths, dtype=torch.int32))
        host = host.reshape(-1).contiguous()
        if host.numel() != B:
            raise RuntimeError(f"lengths has {host.numel()} entries for a batch of {B}")
        if int(host.min()) < 0 or int(host.max()) > T:
            raise RuntimeError(f"lengths must lie in [0, {T}]")
        return host, host.to(device).contiguous()
