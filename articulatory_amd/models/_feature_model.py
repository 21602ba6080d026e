"""``NativeFeatureModel`` — what ``BiGRU`` and ``Transformer`` share: the feature-to-feature models whose modules only HOLD parameters while
the arithmetic runs in ``libhificar.so`` behind one native handle (``hificar_bigru_*`` / ``hificar_xfmr_*`` of include/hificar.h).

Here, once: the handle's state over ``_owner.NativeOwner``'s lifecycle (creation from the host copies, the device hand-over
``*_set_parameters_device`` once a handle has trained, when it is invalidated), the eval-mode input checks and the whole ``forward_lowrate``,
the gradient layout, and the parts of the training step that do not depend on the model: the shape refusals, the dropout offset, the
autograd node's bookkeeping and the running-statistics update.  A model supplies ``_PREFIX`` / ``_NAME``, its parameter holders, ``_device``,
``_make_config``, ``_batch_norms``, ``_stats_shape``, its training workspace and the entry points its training step calls.
"""

import ctypes
import logging

import numpy as np
import torch

from .. import _native
from .._owner import ABSENT, NativeOwner, create_handle, current_stream, scratch


def register_stats(module, stats):
    """``register_stats`` of every model: mean / scale buffers for input normalisation from an .h5 or .npy file."""
    assert stats.endswith(".h5") or stats.endswith(".npy")
    if stats.endswith(".h5"):
        from ..utils.hdf5 import read_hdf5  # h5py when importable, else the built-in reader of plain HDF5 files

        mean = read_hdf5(stats, "mean").reshape(-1)
        scale = read_hdf5(stats, "scale").reshape(-1)
    else:
        arr = np.load(stats)
        mean = arr[0].reshape(-1)
        scale = arr[1].reshape(-1)
    module.register_buffer("mean", torch.from_numpy(np.asarray(mean)).float())
    module.register_buffer("scale", torch.from_numpy(np.asarray(scale)).float())
    logging.info("Successfully registered stats as buffer.")


def _grad_layout(module):
    """[(state_dict key, offset, numel)] of the native gradient buffer (hificar_*_grad_info), cached per handle."""
    cached = module.__dict__.get("_grad_info")
    if cached is not None and cached[0] == id(module._handle):
        return cached[1]
    handle = module._handle
    out = []
    name = ctypes.create_string_buffer(96)
    off, num = ctypes.c_int64(), ctypes.c_int64()
    for i in range(module._fn("_grad_count")(handle)):
        module._call("_grad_info", handle, i, name, ctypes.byref(off), ctypes.byref(num))
        out.append((name.value.decode(), off.value, num.value))
    module.__dict__["_grad_info"] = (id(module._handle), out)
    return out


def _tape_forward(ctx, module, x, p, seed, offset, names, params, **how):
    """``forward`` of a model's autograd node: the training forward with a tape (``module._run_forward_train``; ``how``: the model's own
    keyword), and what the backward pass needs on ``ctx``.  ``module._lens`` (None, or the (host, device) int32 lengths of a ragged batch) is
    read here, at forward time; the tape keeps the lengths for the backward."""
    out, stats, tape, toff = module._run_forward_train(x, p, seed, offset, keep_tape=True, lens=module._lens, **how)
    B, _, T = x.shape
    ctx.module, ctx.names, ctx.tape, ctx.toff, ctx.BT = module, names, tape, toff, (B, T)
    ctx.save_for_backward(*params)  # torch's own version check covers an in-place edit that bumps Parameter._version ...
    ctx.steps_seen = module._steps_seen  # ... and this one a fused optimizer step, which does not
    ctx.mark_non_differentiable(stats)
    return out, stats


def _tape_backward(ctx, dout, launch, skip=()):
    """``backward`` of a model's autograd node.  ``launch(handle, dout pointer, B, T, tail, stream)`` runs the model's backward entry point:
    it takes the training workspace and passes ``tail`` (tape, its size, the gradient buffer, dx or None) where the entry point expects it.
    Parameters whose name ends in one of ``skip`` get no gradient."""
    module = ctx.module
    handle = module._handle
    B, T = ctx.BT
    params = ctx.saved_tensors
    if handle is None or ctx.steps_seen != module._steps_seen:
        raise RuntimeError(f"a {module._NAME} parameter was modified between forward and backward (the backward pass reads the weights the "
                           "forward used)")
    dev = ctx.tape.device
    dout = dout.to(torch.float32).contiguous()
    dx = torch.empty((B, module._params["in_channels"], T), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
    with torch.cuda.device(dev):
        stream = current_stream()
        grads = torch.empty(int(module._fn("_grad_floats")(handle)), dtype=torch.float32, device=dev)
        tail = (ctx.tape.data_ptr() + ctx.toff, ctx.tape.numel() - ctx.toff, grads.data_ptr(), dx.data_ptr() if dx is not None else None)
        launch(handle, dout.data_ptr(), B, T, tail, stream)
    views = {name: grads[off:off + num] for name, off, num in _grad_layout(module)}
    gw = tuple(views[n].view(t.shape) if need and not (skip and n.endswith(skip)) else None
               for n, t, need in zip(ctx.names, params, ctx.needs_input_grad[6:]))
    ctx.tape = None
    return (None, dx, None, None, None, None, *gw)


class NativeFeatureModel(NativeOwner, torch.nn.Module):
    """Base of ``BiGRU`` and ``Transformer``; see the module's docstring."""

    _PREFIX = None     # the C entry points' prefix: "hificar_bigru" / "hificar_xfmr"
    _NAME = None       # the class name in messages
    _DESTROY = property(lambda self: self._PREFIX + "_destroy")
    _ENGINE = property(lambda self: self._PREFIX + "_engine")
    # _on_device: the handle's weights are refreshed from device tensors (set once a training forward ran on it); _dirty: an optimizer
    # stepped since the last hand-over (fused optimizers do not bump Parameter._version)
    _NATIVE = {"_handle": None, "_workspace_buf": None, "_train_ws_buf": None, "_sig": None, "_on_device": False, "_dirty": False,
               "_grad_info": ABSENT}
    # _lens: the lengths of the ragged training forward under way (forward_padded); a model adds its own fields that only hold during a
    # training forward, with their idle values
    _PROCESS = {"_lib": None, "_lens": None}
    _WATCHED = True
    _LOWRATE_TRAINING = ""  # how forward_lowrate's refusal in train() mode ends
    _LOWRATE_RANGE = ""     # what _workspace's refusal of a low-rate shape adds

    def _init_native(self):
        """The handle's state.  Called by the model's ``__init__`` once its parameters exist: the dropout seed is drawn from torch's
        generator behind their initialisation."""
        self._reset_native()
        self._steps_seen = 0     # optimizer steps noticed so far
        self._calls = 0          # training forwards so far: the dropout generator's offset
        # drawn from torch's generator (after the parameters): torch.manual_seed makes a training run repeatable
        self._dropout_seed = int(torch.randint(0, 2 ** 62, (1,), device="cpu").item())  # (the CPU generator, also under torch.device("meta"))

    def _fn(self, suffix):
        return getattr(self._lib, self._PREFIX + suffix)

    def _call(self, suffix, *args):
        """An entry point that returns a status: ``hificar_<model><suffix>(*args)``, checked."""
        what = self._PREFIX + suffix
        _native.check(getattr(self._lib, what)(*args), what)

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
        """Nothing carries weight norm (the reference finds none either); articulatory_amd.bin.decode calls it on every model."""

    def register_stats(self, stats):
        """Register mean/scale buffers for input normalisation, as the reference's ``register_stats`` does."""
        register_stats(self, stats)

    # ------------------------------------------------------------------ native handle
    def native_state(self):
        """{reference state_dict key: fp32 CPU tensor} of what the C ABI consumes (every float tensor but the input statistics)."""
        out = {}
        for k, v in self.state_dict().items():
            if k in ("mean", "scale") or k.endswith("num_batches_tracked"):
                continue
            out[k] = v.detach().float().cpu().contiguous()
        return out

    def _signature(self):
        ts = list(self.parameters())
        for bn in self._batch_norms():
            ts += [bn.running_mean, bn.running_var]
        return tuple((t.data_ptr(), t._version) for t in ts)

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
        """Every float tensor of the state_dict from device memory into the handle (hificar_*_set_parameters_device): nothing goes
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
            self._call("_set_parameters_device", self._handle, arr, ptrs, len(held), current_stream())
        self._on_device = True
        self._dirty = False
        self._sig = self._signature()

    def _finalize_handle(self, handle):
        """From the last ``set_weight`` to the end of the handle's creation; a model with choices to make around ``finalize`` overrides it."""
        self._call("_finalize", handle)

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
            raise RuntimeError("%s: parameters are on %s; the forward only exists as HIP kernels (move the model to a MI355X with "
                               ".to('cuda')). There is no CPU fallback." % (self._NAME, dev))
        self._lib = _native.load_library()
        with torch.cuda.device(dev):
            cfg = self._make_config()
            handle = create_handle(self._lib, self._PREFIX, lambda h: self._call("_create", ctypes.byref(cfg), ctypes.byref(h)),
                                   self.native_state(), self._finalize_handle)
        self._handle = handle
        self._sig = self._signature()
        if train:
            self._send_parameters()
        return handle

    def _workspace(self, B, T, factor=None):
        """One grow-only scratch buffer per model for the eval forward (hificar_*_workspace_bytes; ``factor``: T low-rate frames,
        hificar_*_workspace_bytes_lowrate)."""
        if factor is None:
            n = self._fn("_workspace_bytes")(self._handle, B, T)
        else:
            n = self._fn("_workspace_bytes_lowrate")(self._handle, B, T, factor)
            if n == 0:
                raise RuntimeError(f"{self._NAME}.forward_lowrate: B={B}, Tl={T}, interp_factor={factor} out of range{self._LOWRATE_RANGE}")
        return scratch(self, "_workspace_buf", n, self._device)

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

    # ------------------------------------------------------------------ eval forward
    def _forward_eval(self, what, x, lengths, factor=None, zscore=False):
        """The eval-mode forward ``what``: "forward" (hificar_*_forward) or, with ``factor``, "forward_lowrate" (hificar_*_forward_lowrate, x
        and ``lengths`` at the low rate)."""
        name = f"{self._NAME}.{what}"
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise RuntimeError(f"{name} needs a CUDA/HIP tensor; there is no CPU fallback")
        if x.dim() != 3 or x.shape[1] != self._params["in_channels"]:
            raise RuntimeError(f"{name}: expected (B, {self._params['in_channels']}, {'T' if factor is None else 'Tl'}), got {tuple(x.shape)}")
        handle = self._native_handle()
        if x.device != self._device():
            raise RuntimeError(f"{name}: input on {x.device}, parameters on {self._device()}")
        c = x.detach().to(torch.float32).contiguous()
        B, _, T = c.shape
        if B < 1 or T < 1:
            raise RuntimeError(f"{name}: empty input {tuple(c.shape)}")
        lens = (None, None)
        keep = None
        if lengths is not None:
            keep = self._check_lengths(lengths, B, T, c.device)
            lens = (keep[1].data_ptr(), keep[0].data_ptr())
        low = () if factor is None else (factor, 1 if zscore else 0)
        out = torch.empty((B, self._params["out_channels"], (factor or 1) * T), dtype=torch.float32, device=c.device)
        with torch.cuda.device(c.device):
            ws_ptr, ws_bytes = self._workspace(B, T, factor=factor)
            self._call("_" + what, handle, c.data_ptr(), lens[0], lens[1], out.data_ptr(), B, T, *low, ws_ptr, ws_bytes, current_stream())
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
        materialised (BiGRU: layer 1's input projection runs at the low rate and its pre-gates are interpolated; Transformer: the input rows
        are formed at the model's rate from the low-rate input, at any ``precision``).  ``interp_factor=1, zscore=False`` is
        ``forward(x, lengths=lengths)``."""
        f = _native.check_interp_factor(interp_factor)
        if self.training:
            raise NotImplementedError(f"{self._NAME}.forward_lowrate: the low-rate front end is an inference path (call .eval(); "
                                      f"{self._LOWRATE_TRAINING})")
        return self._forward_eval("forward_lowrate", x, lengths, factor=f, zscore=zscore)

    # ------------------------------------------------------------------ training forward
    def _train_head(self, x, lengths, padded, f=1):
        """The training forward up to the parameters' hand-over, behind the model's own refusals: x is a (B, in_channels, T) tensor on a
        device (``f``: at 1 / f of the model's rate).  Returns (lens, n): the checked (host, device) lengths of a padded batch or None, and the
        number of frames the batch statistics run over."""
        if x.dim() != 3 or x.shape[1] != self._params["in_channels"]:
            raise RuntimeError(f"{self._NAME}.forward: expected (B, {self._params['in_channels']}, T), got {tuple(x.shape)}")
        B, _, T = x.shape
        if B < 1 or T < 1:
            raise RuntimeError(f"{self._NAME}.forward: empty input {tuple(x.shape)}")
        n = B * T * f
        lens = None
        if padded:
            lens = self._check_lengths(lengths, B, T, x.device)
            n = int(lens[0].sum()) * f
        if n < 2:  # torch.nn.functional.batch_norm's own refusal
            width = self._stats_shape()[-1]
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {[B, width, f * T] if lens is None else [n, width]}")
        self._native_handle(train=True)
        if x.device != self._device():
            raise RuntimeError(f"{self._NAME}.forward: input on {x.device}, parameters on {self._device()}")
        return lens, n

    def _train_tail(self, function, x, lens, n, **under_way):
        """The training forward from the dropout offset on.  ``function``: the model's autograd node; ``under_way``: the model's transient
        field (without its underscore) for this forward, also the keyword of its ``_run_forward_train``.  With grad enabled the output is part
        of the autograd graph; without, the same arithmetic runs and its tape is dropped.  Either way the call advances the dropout generator's
        offset and updates every batch norm's running_mean / running_var / num_batches_tracked as torch.nn.BatchNorm1d does.  Returns (out,
        the batch statistics)."""
        x = x.to(torch.float32).contiguous()
        named = list(self.named_parameters())
        names, params = tuple(k for k, _ in named), [p for _, p in named]
        p, seed = self._params["dropout"], self._dropout_seed
        offset = self._calls
        self._calls += 1
        self._lens = lens
        for k, v in under_way.items():
            setattr(self, "_" + k, v)
        try:
            if torch.is_grad_enabled() and (x.requires_grad or any(q.requires_grad for q in params)):
                out, stats = function.apply(self, x, p, seed, offset, names, *params)
            else:  # no graph: the same arithmetic without a tape (tape = NULL)
                out, stats, _, _ = self._run_forward_train(x.detach(), p, seed, offset, keep_tape=False, lens=lens, **under_way)
        finally:
            self._lens = None
            for k in under_way:
                setattr(self, "_" + k, self._PROCESS["_" + k])
        with torch.no_grad():  # torch.nn.BatchNorm1d: momentum 0.1, the running variance takes the UNBIASED batch variance (n: the valid frames)
            per_bn = stats.view(-1, 2, stats.shape[-1])  # (number of batch norms, mean | biased variance, channels)
            for j, bn in enumerate(self._batch_norms()):
                bn.running_mean.mul_(0.9).add_(per_bn[j, 0], alpha=0.1)
                bn.running_var.mul_(0.9).add_(per_bn[j, 1], alpha=0.1 * n / (n - 1))
                bn.num_batches_tracked += 1
        # (the running statistics only enter the eval path: its folds are refreshed when an eval forward next asks for the handle)
        return out, stats
