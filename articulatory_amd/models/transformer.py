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

import math

import torch

from .. import _native
from .._owner import aligned, current_stream, scratch
from ._feature_model import NativeFeatureModel, _grad_layout, _tape_backward, _tape_forward  # noqa: F401  (_grad_layout: imported from here too)
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


class _TransformerFunction(torch.autograd.Function):
    """Autograd node of the native Transformer in train() mode: forward = hificar_xfmr_forward_train (or, with ``module._lens`` set by
    ``forward_padded``, hificar_xfmr_forward_train_ragged: the lengths are read here, at forward time, and live on in the tape), backward =
    hificar_xfmr_backward (``module._packed``: the packed pair of entry points).  Inputs after (module, x, p, seed, offset, names) are the
    module's parameters in ``names`` order.  Returns (out, batch statistics (number of batch norms, 2, hidden_dim): mean | biased variance); the statistics carry no gradient."""

    @staticmethod
    def forward(ctx, module, x, p, seed, offset, names, *params):
        ctx.packed_lens = module._lens[0] if module._packed else None  # the host lengths: hificar_xfmr_backward_packed checks them
        return _tape_forward(ctx, module, x, p, seed, offset, names, params, packed=module._packed)

    @staticmethod
    def backward(ctx, dout, _dstats=None):
        module, packed_lens = ctx.module, ctx.packed_lens

        def launch(handle, dout_ptr, B, T, tail, stream):
            if packed_lens is None:
                module._call("_backward", handle, dout_ptr, B, T, *tail, *module._train_workspace(B, T), stream)
            else:
                module._call("_backward_packed", handle, dout_ptr, packed_lens.data_ptr(), B, T, *tail,
                             *module._train_workspace(B, T, module._packed_rows(packed_lens, B, T)), stream)

        return _tape_backward(ctx, dout, launch, skip=() if module.train_relative_positions else ("relative_positional.embeddings",))


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


class Transformer(NativeFeatureModel, metaclass=_PrecisionKeyword):
    """Three ResBlocks -> Linear -> ``elayers`` post-LayerNorm encoder layers (8 heads, learned relative positions, 3072-wide feed-forward)
    -> Linear; MI355X-native, eval and train().  ``precision="bf16x3"`` (keyword only): see the module's docstring and ``set_precision``."""

    _PREFIX = "hificar_xfmr"
    _NAME = "Transformer"
    # whether the ragged training forward under way is the packed form; this batch's statistics, for inspection
    _PROCESS = {**NativeFeatureModel._PROCESS, "_packed": False, "_last_stats": None}
    _LOWRATE_TRAINING = "training on low-rate inputs is not built"
    _LOWRATE_RANGE = " (B factor Tl 3072 < 2^31)"

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
        self.train_relative_positions = True  # False: the tables get no gradient, as in the reference (see the module's docstring)
        self._init_native()

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

    def _batch_norms(self):
        """The BatchNorm1d holders in registration order: the order of hificar_xfmr_forward_train's bn_batch_stats."""
        out = []
        for blk in self.conv_blocks:
            out += [blk.bn1, blk.bn2]
            if hasattr(blk, "res_norm"):
                out.append(blk.res_norm)
        return out

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

    def _make_config(self):
        return _native.make_xfmr_config(self._params)

    def _stats_shape(self):
        return (len(self._batch_norms()), 2, self._params["hidden_dim"])

    def __setstate__(self, state):
        state.setdefault("train_precision", "f32")  # (a pickle from before the keyword)
        super().__setstate__(state)

    def _finalize_handle(self, handle):
        self._call("_set_precision", handle, _native.XFMR_PRECISIONS[self.precision])
        super()._finalize_handle(handle)
        if self.precision == "f32":  # (a bf16x3 inference handle has no training arithmetic to choose)
            self._call("_set_train_precision", handle, _native.XFMR_TRAIN_PRECISIONS_K[self.train_precision])

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
            n = self._lib.hificar_xfmr_train_workspace_bytes(self._handle, B, T)
        else:
            n = self._lib.hificar_xfmr_train_workspace_bytes_packed(self._handle, B, packed_rows)
        return scratch(self, "_train_ws_buf", n, self._device)

    def _run_forward_train(self, x, p, seed, offset, keep_tape, lens=None, packed=False):
        """hificar_xfmr_forward_train (lens = (host, device) int32 lengths: hificar_xfmr_forward_train_ragged, or, packed,
        hificar_xfmr_forward_train_packed) on the current stream: (out, batch statistics, tape or None, the tape's alignment offset)."""
        lib, handle = self._lib, self._handle
        B, _, T = x.shape
        dev = x.device
        mp = self._packed_rows(lens[0], B, T) if packed else None
        with torch.cuda.device(dev):
            stream = current_stream()
            tape, toff = None, 0
            if keep_tape:
                nbytes = lib.hificar_xfmr_tape_bytes_packed(handle, B, mp) if packed else lib.hificar_xfmr_tape_bytes(handle, B, T)
                tape, ptr = aligned(nbytes, dev)
                toff = ptr - tape.data_ptr()
            out = torch.empty((B, self._params["out_channels"], T), dtype=torch.float32, device=dev)
            stats = torch.empty(self._stats_shape(), dtype=torch.float32, device=dev)
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
        return self._forward_eval("forward", x, lengths)

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
        lens, n = self._train_head(x, lengths, padded)
        if padded and packed:
            self._packed_rows(lens[0], x.shape[0], x.shape[2])  # (a batch too large to pack is refused here, before a mask is drawn)
        out, stats = self._train_tail(_TransformerFunction, x, lens, n, packed=packed and padded)
        self._last_stats = stats.detach()  # (number of batch norms, 2, hidden_dim): this batch's mean | biased variance, for inspection
        return out
