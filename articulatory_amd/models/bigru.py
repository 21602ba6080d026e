"""``BiGRU`` — the speech-to-EMA (articulatory inversion) model behind the reference's ``generator_type`` plugin surface.

Drop-in for ``articulatory.models.BiGRU`` (reference articulatory/models/pytorch_models.py:22-123) in eval mode: same class name,
constructor keywords and defaults, the same state_dict keys, shapes and order — ``gru{1,2}.{weight,bias}_{ih,hh}_l0[_reverse]``,
``fc1.0.*``, ``bn.*`` (``num_batches_tracked`` included), ``fc2.*`` / ``fc2.0.*`` — and the same ``forward`` / ``inference`` /
``register_stats`` / ``remove_weight_norm``.  The modules below only HOLD parameters; the arithmetic runs in ``libhificar.so``
(``hificar_bigru_*`` of include/hificar.h): no PyTorch-operator implementation, no CPU fallback.

In ``train()`` mode the forward is the reference's training-mode forward — ``Dropout(p)`` behind each GRU layer and fc1, ``BatchNorm1d`` on
batch statistics with the running-statistics update — under autograd: ``_BiGRUFunction`` keeps a tape in ``hificar_bigru_forward_train`` and
routes ``hificar_bigru_backward``'s gradients to every parameter (and to the input when it requires grad).  Dropout masks come from the
package's own counter-based generator (``set_dropout_seed``; numpy restatement: ``utils.synth.bigru_dropout_mask``).

``forward_lowrate(x, lengths, interp_factor, zscore)`` is the reference's speech-to-EMA front end (egs/ema/voc1/local/predict_ema.py:83-101:
linear interpolation of low-rate features, per-utterance z-score) and the eval forward in one device call (``hificar_bigru_forward_lowrate``).
``forward_lowrate_train`` is the same front end in front of the training step, under autograd (``hificar_bigru_forward_train_lowrate`` /
``hificar_bigru_backward_lowrate``): the model trains on the low-rate inputs themselves, and their gradient comes back at the low rate.

Not built, refused with ``NotImplementedError``: ``use_ar`` (the reference's own driver for it is broken: predict_ema.py:92 passes a
keyword ``ar_loop`` does not take) and ``use_spk_emb``.  ``lengths=`` is this package's addition for eval mode: a ragged batch in which
every utterance's result is that of running it alone.  ``forward`` in train() mode takes equal-length batches, as the reference's collater
makes them; ``forward_padded(mels, lengths)`` trains on whole utterances of unequal lengths (this package's definition, the reference never
masks: each sequence swept over its own frames, batch statistics, loss and gradients over the valid frames only).
"""

import math

import torch

from .. import _native
from .._owner import aligned, current_stream, scratch
from ._feature_model import NativeFeatureModel, _grad_layout, _tape_backward, _tape_forward  # noqa: F401  (_grad_layout: imported from here too)

FC1_DIM = 128  # pytorch_models.py:32-33


class _GRUParams(torch.nn.Module):
    """Parameter holder with torch.nn.GRU's names and registration order (one bidirectional layer, pytorch_models.py:27-30)."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        k = 1.0 / math.sqrt(hidden_size)  # torch.nn.GRU.reset_parameters
        for sfx in ("", "_reverse"):
            for name, shape in (("weight_ih_l0", (3 * hidden_size, input_size)), ("weight_hh_l0", (3 * hidden_size, hidden_size)),
                                ("bias_ih_l0", (3 * hidden_size,)), ("bias_hh_l0", (3 * hidden_size,))):
                setattr(self, name + sfx, torch.nn.Parameter(torch.empty(shape).uniform_(-k, k)))


class _LinearParams(torch.nn.Module):
    def __init__(self, in_features, out_features):
        super().__init__()
        k = 1.0 / math.sqrt(in_features)  # torch.nn.Linear.reset_parameters
        self.weight = torch.nn.Parameter(torch.empty(out_features, in_features).uniform_(-k, k))
        self.bias = torch.nn.Parameter(torch.empty(out_features).uniform_(-k, k))


class _BatchNormParams(torch.nn.Module):
    """torch.nn.BatchNorm1d's parameters and buffers (pytorch_models.py:33); only the running statistics are ever used."""

    def __init__(self, n):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(n))
        self.bias = torch.nn.Parameter(torch.zeros(n))
        self.register_buffer("running_mean", torch.zeros(n))
        self.register_buffer("running_var", torch.ones(n))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class _BiGRUFunction(torch.autograd.Function):
    """Autograd node of the native BiGRU in train() mode: forward = hificar_bigru_forward_train (keeps a tape), backward =
    hificar_bigru_backward.  Inputs after (module, x, p, seed, offset, names) are the module's parameters in ``names`` order.  Returns
    (out, batch statistics (2, 128): mean | biased variance of the batch norm's input); the statistics carry no gradient.  ``module._lens``
    (None, or the (host, device) int32 lengths of a ragged batch) is read at forward time; the tape keeps the lengths for the backward.
    ``module._low`` (None, or (interp_factor, zscore) of ``forward_lowrate_train``): x is (B, in_channels, Tl) at the low rate, and so is its
    gradient (hificar_bigru_forward_train_lowrate / hificar_bigru_backward_lowrate)."""

    @staticmethod
    def forward(ctx, module, x, p, seed, offset, names, *params):
        ctx.low = module._low
        return _tape_forward(ctx, module, x, p, seed, offset, names, params, low=module._low)

    @staticmethod
    def backward(ctx, dout, _dstats=None):
        module, low = ctx.module, ctx.low

        def launch(handle, dout_ptr, B, T, tail, stream):
            if low is None:
                module._call("_backward", handle, dout_ptr, B, T, *tail, *module._train_workspace(B, T), stream)
            else:  # (T: low-rate frames, as x has them; dx likewise)
                module._call("_backward_lowrate", handle, dout_ptr, B, T, low[0], 1 if low[1] else 0, *tail,
                             *module._train_workspace(B, T, factor=low[0]), stream)

        return _tape_backward(ctx, dout, launch)


class BiGRU(NativeFeatureModel):
    """Two bidirectional GRU layers -> Linear(2H, 128) -> BatchNorm1d(128) -> Linear(128, out) (-> tanh); MI355X-native, eval and train()."""

    _PREFIX = "hificar_bigru"
    _NAME = "BiGRU"
    _PROCESS = {**NativeFeatureModel._PROCESS, "_low": None}  # (interp_factor, zscore) of the low-rate training forward under way
    _LOWRATE_TRAINING = "to train on low-rate inputs call forward_lowrate_train"

    def __init__(self, in_channels=80, hidden_size=256, dropout=0.3, out_channels=1,
                 use_ar=False, ar_input=512, ar_hidden=256, ar_output=128, ar_channels=None, use_tanh=False,
                 use_spk_emb=False, spk_emb_size=32, spk_emb_hidden=32):
        super().__init__()
        if use_ar:
            raise NotImplementedError("BiGRU(use_ar=True) is not built (the reference's own driver for it cannot run: "
                                      "egs/ema/voc1/local/predict_ema.py:92 passes a keyword ar_loop does not take)")
        if use_spk_emb:
            raise NotImplementedError("BiGRU(use_spk_emb=True) is not built")
        self.use_ar = False
        self.use_spk_emb = False
        self._params = dict(in_channels=in_channels, hidden_size=hidden_size, dropout=dropout, out_channels=out_channels, use_tanh=use_tanh)
        _native.check_bigru_params(self._params)  # libhificar's own limits: fail here, not at the first forward on the device
        self.gru1 = _GRUParams(in_channels, hidden_size)
        self.gru2 = _GRUParams(hidden_size * 2, hidden_size)
        self.fc1 = torch.nn.Sequential(_LinearParams(hidden_size * 2, FC1_DIM))  # (+ Dropout in the reference: no parameters)
        self.bn = _BatchNormParams(FC1_DIM)
        self.fc2 = torch.nn.Sequential(_LinearParams(FC1_DIM, out_channels)) if use_tanh else _LinearParams(FC1_DIM, out_channels)
        self._init_native()

    def inference(self, c, normalize_before=True, ar=None, spk=None):
        """(T, in_channels) tensor or ndarray -> (T, out_channels), pytorch_models.py:86-105 statement for statement (a 3-D input is
        taken as (1, in_channels, T); ``normalize_before`` defaults to True here, unlike the generators)."""
        if len(c.shape) == 3:
            c = c.transpose(1, 2)
            c = c[0]
        if not isinstance(c, torch.Tensor):
            c = torch.tensor(c, dtype=torch.float).to(self._device())
        if normalize_before:
            c = (c - self.mean) / self.scale
        c = self.forward(c.unsqueeze(0).transpose(1, 2), ar=ar, spk=spk)
        return c.transpose(1, 2).squeeze(0)

    # ------------------------------------------------------------------ what NativeFeatureModel asks of a model
    def _device(self):
        return self.gru1.weight_ih_l0.device

    def _make_config(self):
        return _native.make_bigru_config(self._params)

    def _batch_norms(self):
        return [self.bn]

    def _stats_shape(self):
        return (2, FC1_DIM)

    def _train_workspace(self, B, T, factor=None):
        """One grow-only scratch buffer shared by the training forward and the backward pass (hificar_bigru_train_workspace_bytes; ``factor``:
        T low-rate frames, hificar_bigru_train_workspace_bytes_lowrate)."""
        if factor is None:
            n = self._lib.hificar_bigru_train_workspace_bytes(self._handle, B, T)
        else:
            n = self._lib.hificar_bigru_train_workspace_bytes_lowrate(self._handle, B, T, factor)
            if n == 0:
                raise RuntimeError(f"BiGRU.forward_lowrate_train: B={B}, Tl={T}, interp_factor={factor} out of range")
        return scratch(self, "_train_ws_buf", n, self._device)

    def _run_forward_train(self, x, p, seed, offset, keep_tape, lens=None, low=None):
        """hificar_bigru_forward_train (lens = (host, device) int32 lengths: hificar_bigru_forward_train_ragged; low = (interp_factor, zscore):
        hificar_bigru_forward_train_lowrate, x and lens at the low rate) on the current stream: (out, batch statistics, tape or None, the
        tape's alignment offset)."""
        lib, handle = self._lib, self._handle
        B, _, T = x.shape
        f = 1 if low is None else low[0]
        dev = x.device
        with torch.cuda.device(dev):
            stream = current_stream()
            tape, toff = None, 0
            if keep_tape:
                n = lib.hificar_bigru_tape_bytes(handle, B, T) if low is None else lib.hificar_bigru_tape_bytes_lowrate(handle, B, T, f)
                tape, ptr = aligned(n, dev)
                toff = ptr - tape.data_ptr()
            out = torch.empty((B, self._params["out_channels"], f * T), dtype=torch.float32, device=dev)
            stats = torch.empty(self._stats_shape(), dtype=torch.float32, device=dev)
            ws_ptr, ws_bytes = self._train_workspace(B, T, factor=None if low is None else f)
            tail = (float(p), seed, offset, tape.data_ptr() + toff if keep_tape else None, tape.numel() - toff if keep_tape else 0,
                    ws_ptr, ws_bytes, stream)
            if low is not None:
                what = "hificar_bigru_forward_train_lowrate"
                rc = lib.hificar_bigru_forward_train_lowrate(handle, x.data_ptr(), None if lens is None else lens[1].data_ptr(),
                                                             None if lens is None else lens[0].data_ptr(), out.data_ptr(), stats.data_ptr(), B, T, f,
                                                             1 if low[1] else 0, *tail)
            elif lens is None:
                what = "hificar_bigru_forward_train"
                rc = lib.hificar_bigru_forward_train(handle, x.data_ptr(), out.data_ptr(), stats.data_ptr(), B, T, *tail)
            else:
                what = "hificar_bigru_forward_train_ragged"
                rc = lib.hificar_bigru_forward_train_ragged(handle, x.data_ptr(), lens[1].data_ptr(), lens[0].data_ptr(), out.data_ptr(),
                                                            stats.data_ptr(), B, T, *tail)
        _native.check(rc, what)
        return out, stats, tape, toff

    # ------------------------------------------------------------------ forward
    def forward(self, mels, mask=None, spk_id=None, spk=None, ar=None, ph=None, lengths=None):
        """mels: (B, in_channels, T) -> EMA (B, out_channels, T)  (pytorch_models.py:45-72, eval mode).  ``mask``, ``spk_id``, ``ph`` (and,
        without use_ar / use_spk_emb, ``ar`` and ``spk``) are accepted and ignored, as in the reference.  ``lengths`` (B frame counts): a
        ragged batch — utterance b is computed as if it were alone with lengths[b] frames (its reverse direction starts at its own last
        frame; zero padding would not be equivalent) and out[b, :, lengths[b]:] is zero."""
        if self.training:
            return self._forward_train(mels, lengths)
        return self._forward_eval("forward", mels, lengths)

    def forward_lowrate_train(self, x, lengths=None, interp_factor=1, zscore=False):
        """Training on low-rate inputs.  eval(): ``forward_lowrate(x, lengths, interp_factor, zscore)``.  train(): x (B, in_channels, Tl) ->
        (B, out_channels, interp_factor * Tl) under autograd, with T = interp_factor * Tl exactly ``forward`` (``lengths=None``) or
        ``forward_padded`` (``lengths``: B LOW-RATE frame counts; sequence b has interp_factor * lengths[b] frames at the model's rate) applied
        to the input stretched as ``forward_lowrate`` describes, every sequence clamped at its own last frame: the dropout masks are those of
        the (B, T, C) tensors, the batch statistics run over M = interp_factor * sum(lengths) rows (M >= 2), the output is zero past
        interp_factor * lengths[b], ``bn.running_*`` and the dropout offset advance as they do there, and with grad disabled the tape-less
        form runs.  The stretched input is never materialised, forwards or backwards: layer 1's projection and its weight and data gradients
        run over the B Tl low-rate rows (the interpolation commutes with them) and the tape keeps low-rate rows.  When ``x`` requires grad its
        gradient is (B, in_channels, Tl), exactly zero on padded low-rate frames; what ``x`` holds there is never read.  ``zscore``: every
        utterance is normalised by its own mean and population standard deviation first, taken as constants: the parameter gradients are
        exact, an ``x`` that requires grad is refused (the statistics' own derivative is not built).  ``interp_factor=1, zscore=False`` is
        ``forward`` / ``forward_padded`` (the same launches)."""
        f = _native.check_interp_factor(interp_factor)
        if not self.training:
            return self.forward_lowrate(x, lengths=lengths, interp_factor=interp_factor, zscore=zscore)
        if zscore and isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("BiGRU.forward_lowrate_train(zscore=True): the gradient of the input is not built (the utterance "
                                      "statistics are taken as constants); detach x")
        if f == 1 and not zscore:
            return self._forward_train(x, lengths, padded=lengths is not None)
        return self._forward_train(x, lengths, padded=lengths is not None, low=(f, bool(zscore)))

    def forward_padded(self, mels, lengths):
        """A batch of whole utterances, zero-padded to (B, in_channels, T), with their frame counts ``lengths`` (B values in 0 .. T).
        eval(): ``forward(mels, lengths=lengths)``.  train(): the training step on the ragged batch, under autograd — this package's
        definition, the reference never masks: sequence b is swept over its own lengths[b] frames (the reverse direction from its own last
        frame), dropout masks are those of the padded tensors (they depend on T), the batch norm takes mean and biased variance over the
        M = sum(lengths) valid frames (running variance: M / (M - 1)), ``out[b, :, lengths[b]:]`` is exactly zero; backwards, the output
        gradient on padded frames is ignored whatever it holds, the input gradient is zero there, and every parameter gradient sums valid
        frames only.  With every length equal to T all results are bitwise those of ``forward``.  What ``mels`` holds in padded frames is
        never used."""
        if not self.training:
            return self.forward(mels, lengths=lengths)
        if lengths is None:
            raise RuntimeError("BiGRU.forward_padded needs lengths")
        return self._forward_train(mels, lengths, padded=True)

    def _forward_train(self, mels, lengths, padded=False, low=None):
        """train() mode (pytorch_models.py:45-72 with its three nn.Dropout active and the batch norm on batch statistics): with grad enabled
        the output is part of the autograd graph; without, the same arithmetic runs and its tape is dropped.  Every call — either way —
        advances the dropout generator's offset and updates bn.running_mean / running_var / num_batches_tracked as torch.nn.BatchNorm1d does."""
        if lengths is not None and not padded:
            raise NotImplementedError("BiGRU.forward(lengths=...) in train() mode is refused: masked batch statistics are this package's "
                                      "definition, not the reference's, so asking for them is explicit: call forward_padded(mels, lengths) "
                                      "to train on a ragged batch (or .eval() for ragged inference)")
        if not isinstance(mels, torch.Tensor) or mels.device.type != "cuda":
            raise NotImplementedError("BiGRU.forward in train() mode needs a CUDA/HIP tensor: the training path only exists as HIP kernels "
                                      "(there is no CPU fallback)")
        # (low: mels and lengths are at the low rate, T low-rate frames; the model sees f T)
        lens, n = self._train_head(mels, lengths, padded, f=1 if low is None else low[0])
        return self._train_tail(_BiGRUFunction, mels, lens, n, low=low)[0]
