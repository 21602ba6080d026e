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

import ctypes
import logging
import math

import numpy as np
import torch

from .. import _native

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


def _grad_layout(module):
    """[(state_dict key, offset, numel)] of the native gradient buffer (hificar_bigru_grad_info), cached per handle."""
    cached = module.__dict__.get("_grad_info")
    if cached is not None and cached[0] == id(module._handle):
        return cached[1]
    lib, handle = module._lib, module._handle
    out = []
    name = ctypes.create_string_buffer(96)
    off, num = ctypes.c_int64(), ctypes.c_int64()
    for i in range(lib.hificar_bigru_grad_count(handle)):
        _native.check(lib.hificar_bigru_grad_info(handle, i, name, ctypes.byref(off), ctypes.byref(num)), "hificar_bigru_grad_info")
        out.append((name.value.decode(), off.value, num.value))
    module.__dict__["_grad_info"] = (id(module._handle), out)
    return out


class _BiGRUFunction(torch.autograd.Function):
    """Autograd node of the native BiGRU in train() mode: forward = hificar_bigru_forward_train (keeps a tape), backward =
    hificar_bigru_backward.  Inputs after (module, x, p, seed, offset, names) are the module's parameters in ``names`` order.  Returns
    (out, batch statistics (2, 128): mean | biased variance of the batch norm's input); the statistics carry no gradient.  ``module._lens``
    (None, or the (host, device) int32 lengths of a ragged batch) is read at forward time; the tape keeps the lengths for the backward.
    ``module._low`` (None, or (interp_factor, zscore) of ``forward_lowrate_train``): x is (B, in_channels, Tl) at the low rate, and so is its
    gradient (hificar_bigru_forward_train_lowrate / hificar_bigru_backward_lowrate)."""

    @staticmethod
    def forward(ctx, module, x, p, seed, offset, names, *params):
        out, stats, tape, toff = module._run_forward_train(x, p, seed, offset, keep_tape=True, lens=module._lens, low=module._low)
        B, _, T = x.shape
        ctx.module, ctx.names, ctx.tape, ctx.toff, ctx.BT, ctx.low = module, names, tape, toff, (B, T), module._low
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
            raise RuntimeError("a BiGRU parameter was modified between forward and backward (the backward pass reads the weights the "
                               "forward used)")
        dev = ctx.tape.device
        dout = dout.to(torch.float32).contiguous()
        p = module._params
        dx = torch.empty((B, p["in_channels"], T), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            grads = torch.empty(int(lib.hificar_bigru_grad_floats(handle)), dtype=torch.float32, device=dev)
            tail = (ctx.tape.data_ptr() + ctx.toff, ctx.tape.numel() - ctx.toff, grads.data_ptr(), dx.data_ptr() if dx is not None else None)
            if ctx.low is None:
                ws_ptr, ws_bytes = module._train_workspace(B, T)
                rc = lib.hificar_bigru_backward(handle, dout.data_ptr(), B, T, *tail, ws_ptr, ws_bytes, stream)
            else:  # (T: low-rate frames, as x has them; dx likewise)
                ws_ptr, ws_bytes = module._train_workspace(B, T, factor=ctx.low[0])
                rc = lib.hificar_bigru_backward_lowrate(handle, dout.data_ptr(), B, T, ctx.low[0], 1 if ctx.low[1] else 0, *tail, ws_ptr, ws_bytes, stream)
        _native.check(rc, "hificar_bigru_backward" if ctx.low is None else "hificar_bigru_backward_lowrate")
        views = {name: grads[off:off + num] for name, off, num in _grad_layout(module)}
        gw = tuple(views[n].view(t.shape) if need else None for n, t, need in zip(ctx.names, params, ctx.needs_input_grad[6:]))
        ctx.tape = None
        return (None, dx, None, None, None, None, *gw)


class BiGRU(torch.nn.Module):
    """Two bidirectional GRU layers -> Linear(2H, 128) -> BatchNorm1d(128) -> Linear(128, out) (-> tanh); MI355X-native, eval and train()."""

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
        self._low = None         # (interp_factor, zscore) of the low-rate training forward under way (forward_lowrate_train)
        # drawn from torch's generator (after the parameters): torch.manual_seed makes a training run repeatable
        self._dropout_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        from ..utils.optim_hook import watch

        watch(self)  # fused optimizers do not bump Parameter._version: every optimizer.step() over these parameters marks them stale

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

    # ------------------------------------------------------------------ reference surface
    def remove_weight_norm(self):
        """Nothing carries weight norm (pytorch_models.py:74-84 finds none either); articulatory_amd.bin.decode calls it on every model."""

    def register_stats(self, stats):
        """Register mean/scale buffers for input normalisation (pytorch_models.py:107-123)."""
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

    # ------------------------------------------------------------------ native handle
    def _device(self):
        return self.gru1.weight_ih_l0.device

    def native_state(self):
        """{reference state_dict key: fp32 CPU tensor} of what the C ABI consumes (every float tensor but the input statistics)."""
        out = {}
        for k, v in self.state_dict().items():
            if k in ("mean", "scale") or k.endswith("num_batches_tracked"):
                continue
            out[k] = v.detach().float().cpu().contiguous()
        return out

    def _signature(self):
        ts = list(self.parameters()) + [self.bn.running_mean, self.bn.running_var]
        return tuple((t.data_ptr(), t._version) for t in ts)

    def _invalidate(self):
        h = self.__dict__.get("_handle")
        if h is not None and self._lib is not None:
            self._lib.hificar_bigru_destroy(h)
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
        for k in ("_handle", "_lib", "_workspace_buf", "_sig", "_train_ws_buf"):
            state[k] = None
        state["_on_device"] = state["_dirty"] = False
        state.pop("_grad_info", None)
        return state

    def __setstate__(self, state):
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
        """Every float tensor of the state_dict from device memory into the handle (hificar_bigru_set_parameters_device): nothing goes
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
            _native.check(self._lib.hificar_bigru_set_parameters_device(self._handle, arr, ptrs, len(held), stream),
                          "hificar_bigru_set_parameters_device")
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
            raise RuntimeError("BiGRU: parameters are on %s; the forward only exists as HIP kernels (move the model to a MI355X with "
                               ".to('cuda')). There is no CPU fallback." % (dev,))
        lib = _native.load_library()
        self._lib = lib
        handle = ctypes.c_void_p()
        with torch.cuda.device(dev):
            cfg = _native.make_bigru_config(self._params)
            _native.check(lib.hificar_bigru_create(ctypes.byref(cfg), ctypes.byref(handle)), "hificar_bigru_create")
            try:
                for name, t in self.native_state().items():
                    shape = (ctypes.c_int64 * t.dim())(*t.shape)
                    _native.check(lib.hificar_bigru_set_weight(handle, name.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim()),
                                  "hificar_bigru_set_weight")
                _native.check(lib.hificar_bigru_finalize(handle), "hificar_bigru_finalize")
            except Exception:
                lib.hificar_bigru_destroy(handle)
                raise
        self._handle = handle
        self._sig = self._signature()
        if train:
            self._send_parameters()
        return handle

    def _train_workspace(self, B, T, factor=None):
        """One grow-only scratch buffer shared by the training forward and the backward pass (hificar_bigru_train_workspace_bytes; ``factor``:
        T low-rate frames, hificar_bigru_train_workspace_bytes_lowrate)."""
        if factor is None:
            n = self._lib.hificar_bigru_train_workspace_bytes(self._handle, B, T) + 256
        else:
            n = self._lib.hificar_bigru_train_workspace_bytes_lowrate(self._handle, B, T, factor)
            if n == 0:
                raise RuntimeError(f"BiGRU.forward_lowrate_train: B={B}, Tl={T}, interp_factor={factor} out of range")
            n += 256
        ws = self._train_ws_buf
        if ws is None or ws.numel() < n:
            ws = torch.empty(int(n * 1.25) if ws is not None else n, dtype=torch.uint8, device=self._device())
            self._train_ws_buf = ws
        off = (-ws.data_ptr()) % 256
        return ws.data_ptr() + off, ws.numel() - off

    def _run_forward_train(self, x, p, seed, offset, keep_tape, lens=None, low=None):
        """hificar_bigru_forward_train (lens = (host, device) int32 lengths: hificar_bigru_forward_train_ragged; low = (interp_factor, zscore):
        hificar_bigru_forward_train_lowrate, x and lens at the low rate) on the current stream: (out, batch statistics, tape or None, the
        tape's alignment offset)."""
        lib, handle = self._lib, self._handle
        B, _, T = x.shape
        f = 1 if low is None else low[0]
        dev = x.device
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            tape, toff = None, 0
            if keep_tape:
                n = lib.hificar_bigru_tape_bytes(handle, B, T) if low is None else lib.hificar_bigru_tape_bytes_lowrate(handle, B, T, f)
                tape = torch.empty(n + 256, dtype=torch.uint8, device=dev)
                toff = (-tape.data_ptr()) % 256
            out = torch.empty((B, self._params["out_channels"], f * T), dtype=torch.float32, device=dev)
            stats = torch.empty((2, FC1_DIM), dtype=torch.float32, device=dev)
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

    def _workspace(self, B, T, factor=None):
        """One grow-only scratch buffer per model (pre-gates of B x T frames + one row buffer: hificar_bigru_workspace_bytes; ``factor``:
        T low-rate frames, hificar_bigru_workspace_bytes_lowrate)."""
        if factor is None:
            n = self._lib.hificar_bigru_workspace_bytes(self._handle, B, T) + 256
        else:
            n = self._lib.hificar_bigru_workspace_bytes_lowrate(self._handle, B, T, factor)
            if n == 0:
                raise RuntimeError(f"BiGRU.forward_lowrate: B={B}, Tl={T}, interp_factor={factor} out of range")
            n += 256
        ws = self._workspace_buf
        if ws is None or ws.numel() < n:
            # work already enqueued on the old buffer keeps it alive through the caching allocator's stream ordering
            ws = torch.empty(int(n * 1.25) if ws is not None else n, dtype=torch.uint8, device=self._device())
            self._workspace_buf = ws
        off = (-ws.data_ptr()) % 256
        return ws.data_ptr() + off, ws.numel() - off

    def engine(self):
        """The engine handle for ``hificar_profile_begin`` / ``hificar_profile_end`` (per-kernel device times; tools/bigru_bench.py)."""
        handle = self._native_handle()  # first: it is what loads self._lib
        return ctypes.c_void_p(self._lib.hificar_bigru_engine(handle))

    # ------------------------------------------------------------------ forward
    def forward(self, mels, mask=None, spk_id=None, spk=None, ar=None, ph=None, lengths=None):
        """mels: (B, in_channels, T) -> EMA (B, out_channels, T)  (pytorch_models.py:45-72, eval mode).  ``mask``, ``spk_id``, ``ph`` (and,
        without use_ar / use_spk_emb, ``ar`` and ``spk``) are accepted and ignored, as in the reference.  ``lengths`` (B frame counts): a
        ragged batch — utterance b is computed as if it were alone with lengths[b] frames (its reverse direction starts at its own last
        frame; zero padding would not be equivalent) and out[b, :, lengths[b]:] is zero."""
        if self.training:
            return self._forward_train(mels, lengths)
        if not isinstance(mels, torch.Tensor) or mels.device.type != "cuda":
            raise RuntimeError("BiGRU.forward needs a CUDA/HIP tensor; there is no CPU fallback")
        if mels.dim() != 3 or mels.shape[1] != self._params["in_channels"]:
            raise RuntimeError(f"BiGRU.forward: expected (B, {self._params['in_channels']}, T), got {tuple(mels.shape)}")
        handle = self._native_handle()
        if mels.device != self._device():
            raise RuntimeError(f"BiGRU.forward: input on {mels.device}, parameters on {self._device()}")
        c = mels.detach().to(torch.float32).contiguous()
        B, _, T = c.shape
        if B < 1 or T < 1:
            raise RuntimeError(f"BiGRU.forward: empty input {tuple(c.shape)}")
        lens = (None, None)
        keep = None
        if lengths is not None:
            keep = self._check_lengths(lengths, B, T, c.device)
            lens = (keep[1].data_ptr(), keep[0].data_ptr())
        out = torch.empty((B, self._params["out_channels"], T), dtype=torch.float32, device=c.device)
        with torch.cuda.device(c.device):
            ws_ptr, ws_bytes = self._workspace(B, T)
            stream = torch.cuda.current_stream().cuda_stream
            rc = self._lib.hificar_bigru_forward(handle, c.data_ptr(), lens[0], lens[1], out.data_ptr(), B, T, ws_ptr, ws_bytes,
                                                 ctypes.c_void_p(stream))
        _native.check(rc, "hificar_bigru_forward")
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
        materialised: layer 1's input projection runs at the low rate and its pre-gates are interpolated.  ``interp_factor=1, zscore=False`` is ``forward(x, lengths=lengths)``."""
        f = _native.check_interp_factor(interp_factor)
        if self.training:
            raise NotImplementedError("BiGRU.forward_lowrate: the low-rate front end is an inference path (call .eval(); to train on "
                                      "low-rate inputs call forward_lowrate_train)")
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise RuntimeError("BiGRU.forward_lowrate needs a CUDA/HIP tensor; there is no CPU fallback")
        if x.dim() != 3 or x.shape[1] != self._params["in_channels"]:
            raise RuntimeError(f"BiGRU.forward_lowrate: expected (B, {self._params['in_channels']}, Tl), got {tuple(x.shape)}")
        handle = self._native_handle()
        if x.device != self._device():
            raise RuntimeError(f"BiGRU.forward_lowrate: input on {x.device}, parameters on {self._device()}")
        c = x.detach().to(torch.float32).contiguous()
        B, _, Tl = c.shape
        if B < 1 or Tl < 1:
            raise RuntimeError(f"BiGRU.forward_lowrate: empty input {tuple(c.shape)}")
        lens = (None, None)
        keep = None
        if lengths is not None:
            keep = self._check_lengths(lengths, B, Tl, c.device)
            lens = (keep[1].data_ptr(), keep[0].data_ptr())
        out = torch.empty((B, self._params["out_channels"], f * Tl), dtype=torch.float32, device=c.device)
        with torch.cuda.device(c.device):
            ws_ptr, ws_bytes = self._workspace(B, Tl, factor=f)
            stream = torch.cuda.current_stream().cuda_stream
            rc = self._lib.hificar_bigru_forward_lowrate(handle, c.data_ptr(), lens[0], lens[1], out.data_ptr(), B, Tl, f, 1 if zscore else 0, ws_ptr,
                                            ws_bytes, ctypes.c_void_p(stream))
        _native.check(rc, "hificar_bigru_forward_lowrate")
        return out

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
        if mels.dim() != 3 or mels.shape[1] != self._params["in_channels"]:
            raise RuntimeError(f"BiGRU.forward: expected (B, {self._params['in_channels']}, T), got {tuple(mels.shape)}")
        B, _, T = mels.shape
        if B < 1 or T < 1:
            raise RuntimeError(f"BiGRU.forward: empty input {tuple(mels.shape)}")
        f = 1 if low is None else low[0]  # (low: mels and lengths are at the low rate, T low-rate frames; the model sees f T)
        n = B * T * f
        lens = None
        if padded:
            lens = self._check_lengths(lengths, B, T, mels.device)
            n = int(lens[0].sum()) * f
        if n < 2:  # torch.nn.functional.batch_norm's own refusal
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {[B, FC1_DIM, f * T] if lens is None else [n, FC1_DIM]}")
        self._native_handle(train=True)
        if mels.device != self._device():
            raise RuntimeError(f"BiGRU.forward: input on {mels.device}, parameters on {self._device()}")
        x = mels.to(torch.float32).contiguous()
        named = list(self.named_parameters())
        names, params = tuple(n for n, _ in named), [p for _, p in named]
        offset = self._calls
        self._calls += 1
        self._lens, self._low = lens, low
        try:
            if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
                out, stats = _BiGRUFunction.apply(self, x, self._params["dropout"], self._dropout_seed, offset, names, *params)
            else:  # no graph: the same arithmetic without a tape (tape = NULL)
                out, stats, _, _ = self._run_forward_train(x.detach(), self._params["dropout"], self._dropout_seed, offset, keep_tape=False, lens=lens,
                                                           low=low)
        finally:
            self._lens = self._low = None
        with torch.no_grad():  # torch.nn.BatchNorm1d: momentum 0.1, the running variance takes the UNBIASED batch variance (n: the valid frames)
            self.bn.running_mean.mul_(0.9).add_(stats[0], alpha=0.1)
            self.bn.running_var.mul_(0.9).add_(stats[1], alpha=0.1 * n / (n - 1))
            self.bn.num_batches_tracked += 1
        # (the running statistics only enter the eval path: its fold is refreshed when an eval forward next asks for the handle)
        return out
