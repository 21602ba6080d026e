"""``Transformer`` — the feature-to-feature encoder (EMA -> mel and the like) behind the reference's ``generator_type`` plugin surface.

Drop-in for ``articulatory.models.Transformer`` (reference articulatory/models/transformer.py:21-105) in eval mode: same class name,
constructor keywords and defaults, the same state_dict keys, shapes and order — ``conv_blocks.N.{conv1,bn1,conv2,bn2,residual_path,res_norm}.*``
(the batch norms' buffers included), ``w_raw_in.*``, ``transformer.layers.N.self_attn.{w_q,w_k,w_v,w_o}``,
``...self_attn.relative_positional.embeddings``, ``linear1/2``, ``norm1/2``, ``w_out.*`` — and the same ``forward`` / ``inference`` /
``register_stats`` / ``remove_weight_norm``.  The modules below only HOLD parameters; the arithmetic runs in ``libhificar.so``
(``hificar_xfmr_*`` of include/hificar.h): no PyTorch-operator implementation, no CPU fallback.

Not built, refused with ``NotImplementedError``: training (``forward`` in train() mode), ``extra_art=True`` and ``num_ph`` (phoneme input).
``dropout`` and the ``use_ar`` / ``ar_*`` / ``use_tanh`` / ``ph_emb_size`` keywords are accepted and unused, as in the reference.
``lengths=`` is this package's addition: a ragged batch in which every utterance's result is that of running it alone.
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


class Transformer(torch.nn.Module):
    """Three ResBlocks -> Linear -> ``elayers`` post-LayerNorm encoder layers (8 heads, learned relative positions, 3072-wide feed-forward)
    -> Linear; MI355X-native, eval mode."""

    def __init__(self, in_channels=8, out_channels=80, elayers=6, hidden_dim=768, dropout=.2, extra_art=False,
                 use_ar=False, ar_input=512, ar_hidden=256, ar_output=128, use_tanh=False,
                 num_ph=None, ph_emb_size=8, layer_type='default'):
        super().__init__()
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
        self._sig = None

    def __del__(self):
        try:
            self._invalidate()
        except Exception:
            pass

    def __getstate__(self):  # copies and pickles never share a native handle
        state = self.__dict__.copy()
        for k in ("_handle", "_lib", "_workspace_buf", "_sig"):
            state[k] = None
        return state

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

    def _native_handle(self):
        if self._handle is not None and self._sig == self._signature():
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
                _native.check(lib.hificar_xfmr_finalize(handle), "hificar_xfmr_finalize")
            except Exception:
                lib.hificar_xfmr_destroy(handle)
                raise
        self._handle = handle
        self._sig = self._signature()
        return handle

    def _workspace(self, B, T):
        """One grow-only scratch buffer per model (hificar_xfmr_workspace_bytes)."""
        n = self._lib.hificar_xfmr_workspace_bytes(self._handle, B, T) + 256
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
        "layers.N" — as rows (B, T, hidden_dim) into the float32 CUDA tensor ``dst``; ``dst=None`` forgets it, ``name=None`` all of them."""
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
            raise NotImplementedError("Transformer.forward in train() mode is not built (no backward pass, dropout or batch statistics): "
                                      "call .eval() for inference")
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
