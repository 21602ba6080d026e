"""Speech features on the device: ``MFCC`` — what the reference's ``egs/ema/voc1/local/predict_ema.py:32-33`` takes from
``librosa.feature.mfcc`` in front of its MFCC inversion models — and ``LogMel`` — the log-mel filterbank of
``articulatory/bin/preprocess.py:26-82``, the 80-channel input ``BiGRU()`` defaults to.  Both are ``torch.nn.Module``s without parameters over
one native handle (``hificar_feat_*`` of include/hificar.h): waveforms on the device in, features on the device out, ragged batches with
every utterance computed as if alone.  MI355X-native; there is no CPU fallback and no backward.

The arithmetic restates librosa 0.8.1's published algorithm (``stft(center=True, pad_mode="reflect")``, the Slaney filterbank of
``utils.mel``, ``power_to_db``, ``scipy.fftpack.dct(type=2, norm="ortho")``); librosa is not a dependency and parity with it is not pinned.
The z-score of ``wav2mfcc`` is not part of ``MFCC``: ``model.forward_lowrate(feats, lengths=frames, interp_factor=1, zscore=True)`` does it.

``HuBERT`` — the speech model in front of the reference's SSL inversion models (``*_h2``) — has the same call shape but owns parameters: a
``torch.nn.Module`` with the ``transformers`` library's ``HubertModel`` state_dict over a ``hificar_hubert_*`` handle (below).  ``WavLM`` is the
same encoder with WavLM-large's gated relative position bias (``WavLMModel``'s state_dict), the speech model of the reference's
``egs/ema/voc1/local/linear_inference.py``; ``ssl_encoder_from_pretrained`` picks the class by a directory's ``config.json``, and ``LinearHead``
is that script's fitted linear regression on the device.
"""

import ctypes

import numpy as np
import torch

from . import _native
from ._owner import NativeOwner, current_stream, scratch
from .models import _feature_model
from .utils.mel import mel_filterbank


class _SpeechFeature(NativeOwner, torch.nn.Module):
    """What ``MFCC`` and ``LogMel`` share: the native handle (made on first use, never shared by copies or pickles), the grow-only workspace
    and the call."""

    _NAME = None
    _DESTROY = "hificar_feat_destroy"
    _NATIVE = {"_handle": None, "_handle_dev": None, "_workspace_buf": None}

    def _init_native(self, cfg, melmat, channels):
        if cfg.fft_size < 32 or cfg.fft_size % 32:
            raise ValueError(f"{self._NAME}: the FFT size must be a multiple of 32, got {cfg.fft_size}")
        if cfg.hop_size < 1 or not 1 <= cfg.win_length <= cfg.fft_size:
            raise ValueError(f"{self._NAME}: need hop >= 1 and 1 <= win_length <= FFT size, got {cfg.hop_size}, {cfg.win_length}")
        if not 1 <= cfg.num_mels <= _native.FEAT_MAX_MELS:
            raise ValueError(f"{self._NAME}: 1 .. {_native.FEAT_MAX_MELS} mel bands are built, got {cfg.num_mels}")
        self._cfg = cfg
        self.melmat = np.ascontiguousarray(melmat, dtype=np.float32)
        self.channels = channels
        self._reset_native()

    @property
    def fft_size(self):
        return self._cfg.fft_size

    @property
    def hop_size(self):
        return self._cfg.hop_size

    def frames(self, length):
        """Frames of an utterance of ``length`` samples: ``1 + length // hop`` (``librosa.stft(center=True)``)."""
        return 1 + int(length) // self._cfg.hop_size

    def _native_handle(self, dev):
        if self._handle is not None and self._handle_dev != dev:  # (the handle's device state lives where its first forward ran)
            self._invalidate()
        if self._handle is None:
            self._lib = _native.load_library()
            handle = ctypes.c_void_p()
            _native.check(self._lib.hificar_feat_create(ctypes.byref(self._cfg), self.melmat.ctypes.data_as(ctypes.c_void_p), ctypes.byref(handle)),
                          "hificar_feat_create")
            self._handle, self._handle_dev = handle, dev
        return self._handle

    def engine(self):
        """The engine handle for ``hificar_profile_begin`` / ``hificar_profile_end`` (per-kernel device times; tools/features_bench.py),
        once a forward has run (it is what binds the handle to a device)."""
        if self._handle is None:
            raise RuntimeError(f"{self._NAME}.engine: no native handle yet; run a forward first")
        return ctypes.c_void_p(self._lib.hificar_feat_engine(self._handle))

    def forward(self, wav, lengths=None):
        """wav: (B, L) or (L,) float tensor on the device; lengths: B sample counts in 0 < l <= L, or None (every utterance has L).
        Returns (feats (B, C, T) float32 with T = 1 + L // hop, exactly zero from an utterance's own frame count on; frames (B,) int32 on
        the device, ``1 + lengths // hop``)."""
        name = self._NAME
        if not isinstance(wav, torch.Tensor) or wav.device.type != "cuda":
            raise RuntimeError(f"{name} needs a CUDA/HIP tensor; there is no CPU fallback")
        if wav.requires_grad:
            raise RuntimeError(f"{name}: wav requires grad, and no backward through the features is built (detach it)")
        if wav.dim() not in (1, 2) or not wav.is_floating_point():
            raise RuntimeError(f"{name}: expected a (B, L) or (L,) float tensor, got {tuple(wav.shape)} {wav.dtype}")
        y = wav.reshape(1, -1) if wav.dim() == 1 else wav
        y = y.to(torch.float32).contiguous()
        B, L = y.shape
        half = self._cfg.fft_size // 2
        if B < 1:
            raise RuntimeError(f"{name}: empty batch {tuple(wav.shape)}")
        if L <= half:
            raise ValueError(f"{name}: reflect padding needs more than n_fft / 2 = {half} samples, got {L}")
        lens = (None, None)
        keep = None
        if lengths is not None:
            host = lengths.detach().to("cpu", torch.int32) if isinstance(lengths, torch.Tensor) else torch.as_tensor(lengths, dtype=torch.int32)
            host = host.reshape(-1).contiguous()
            if host.numel() != B:
                raise RuntimeError(f"{name}: lengths has {host.numel()} entries for a batch of {B}")
            if int(host.max()) > L or int(host.min()) < 1:
                raise RuntimeError(f"{name}: lengths must lie in [1, {L}]")
            if int(host.min()) <= half:
                raise ValueError(f"{name}: reflect padding needs more than n_fft / 2 = {half} samples, got a length of {int(host.min())}")
            keep = (host, host.to(y.device))
            lens = (keep[1].data_ptr(), keep[0].data_ptr())
        handle = self._native_handle(y.device)
        lib = self._lib
        T = 1 + L // self._cfg.hop_size
        with torch.cuda.device(y.device):
            n = int(lib.hificar_feat_workspace_bytes(handle, B, L))
            if n == 0:
                raise RuntimeError(f"{name}: B={B}, L={L} out of range (B frames n_fft < 2^31, B <= 65535)")
            ws_ptr, ws_bytes = scratch(self, "_workspace_buf", n, y.device)
            out = torch.empty((B, self.channels, T), dtype=torch.float32, device=y.device)
            frames = torch.empty((B,), dtype=torch.int32, device=y.device)
            rc = lib.hificar_feat_forward(handle, y.data_ptr(), lens[0], lens[1], out.data_ptr(), frames.data_ptr(), B, L, ws_ptr, ws_bytes,
                                          current_stream())
        _native.check(rc, "hificar_feat_forward")
        del keep
        return out, frames


class MFCC(_SpeechFeature):
    """``librosa.feature.mfcc(y, sr, n_mfcc, n_fft=, hop_length=, n_mels=)`` of librosa 0.8.1 with ``wav2mfcc``'s defaults
    (predict_ema.py:32-33): power mel spectrogram, ``power_to_db`` (amin 1e-10, top_db 80 under the utterance's own maximum), orthonormal
    DCT-II, the first ``n_mfcc`` coefficients.  ``forward(wav, lengths=None) -> (feats (B, n_mfcc, T), frames (B,))``."""

    _NAME = "MFCC"

    def __init__(self, sampling_rate=16000, n_mfcc=13, n_mels=40, n_fft=320, hop_length=160):
        super().__init__()
        if not 1 <= n_mfcc <= n_mels:
            raise ValueError(f"MFCC: n_mfcc must lie in 1 .. n_mels = {n_mels}, got {n_mfcc}")
        self.sampling_rate = sampling_rate
        melmat = mel_filterbank(sampling_rate, n_fft, n_mels, 0.0, sampling_rate / 2)
        self._init_native(_native.HificarFeatConfig(_native.FEAT_MFCC, n_fft, hop_length, n_fft, n_mels, n_mfcc, 1e-10, 80.0, 10), melmat, n_mfcc)


class LogMel(_SpeechFeature):
    """``logmelfilterbank`` of the reference's ``articulatory/bin/preprocess.py:26-82``, keyword for keyword:
    ``log_b(max(eps, mel_basis |STFT|))``.  ``forward(wav, lengths=None) -> (feats (B, num_mels, T), frames (B,))`` — channels first, as the
    models take them (the reference's function returns (frames, num_mels))."""

    _NAME = "LogMel"

    def __init__(self, sampling_rate, fft_size=1024, hop_size=256, win_length=None, window="hann", num_mels=80, fmin=None, fmax=None, eps=1e-10,
                 log_base=10.0):
        super().__init__()
        if window != "hann":
            raise NotImplementedError(f"LogMel: window='{window}' is not built (only 'hann')")
        if log_base not in (None, 2.0, 10.0):
            raise ValueError(f"{log_base} is not supported.")
        if not eps > 0:
            raise ValueError(f"LogMel: eps must be positive, got {eps}")
        self.sampling_rate = sampling_rate
        fmin = 0 if fmin is None else fmin
        fmax = sampling_rate / 2 if fmax is None else fmax
        melmat = mel_filterbank(sampling_rate, fft_size, num_mels, fmin, fmax)
        cfg = _native.HificarFeatConfig(_native.FEAT_LOGMEL, fft_size, hop_size, fft_size if win_length is None else win_length, num_mels, 0,
                                        eps, -1.0, 0 if log_base is None else int(log_base))
        self._init_native(cfg, melmat, num_mels)


class _Holder(torch.nn.Module):
    """A module that only holds sub-modules by name (the ``HubertModel`` hierarchy's inner nodes)."""

    def __init__(self, **children):
        super().__init__()
        for k, v in children.items():
            setattr(self, k, v)


_WEIGHT_NORM_OLD = {"weight_g": "parametrizations.weight.original0", "weight_v": "parametrizations.weight.original1"}


class HuBERT(_feature_model.NativeFeatureModel):
    """The HuBERT encoder of the "large" family (layer-norm extractor, stable layer norm: ``hubert-large-ll60k``'s architecture), the speech
    model the reference's ``egs/ema/voc1/local/predict_ema.py`` puts in front of its SSL inversion models.  The module owns the parameters —
    ``state_dict()`` has the keys and shapes of the ``transformers`` library's ``HubertModel`` and loads with ``strict=True``; the positional
    conv's weight norm is also accepted in its old form, ``weight_g`` / ``weight_v`` — while the arithmetic runs in ``libhificar.so`` behind one
    native handle (``hificar_hubert_*`` of include/hificar.h): copies and pickles never share a handle, there is no CPU fallback and no
    backward.  Inference only (``eval()`` mode, which the constructor sets); exact fp32 by default.

        feats, frames = hubert(wav, lengths=samples, layer=-1)          # (B, hidden_size, Tmax) at 50 Hz, (B,) int32
        ema = model.forward_lowrate(feats, lengths=frames, interp_factor=4)

    ``wav`` is (B, L) or (L,) at 16 kHz on the device, zero-padded; every utterance is computed as if alone, bit for bit, and ``feats`` is
    exactly zero from an utterance's own ``frames(l) = (l - 400) // 320 + 1`` on.  ``layer=-1`` is the last hidden state (behind the encoder's
    ``layer_norm``), ``layer=k`` in 0 .. N - 1 the library's ``hidden_states[k]``; layers k and above are then not run.

    ``normalize`` (default on): every utterance is first brought to zero mean and unit variance over its own samples,
    ``(x - mean) / sqrt(var + norm_eps)`` with the population variance, inside the first kernel's reads.  ``norm_eps`` defaults to 1e-7, the
    constant of the library's ``Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm``.  The reference's s3prl pipeline normalises with
    ``F.layer_norm`` over the waveform, whose eps is 1e-5 as far as is known here — s3prl is not on hand to check — so it is a field.

    ``precision`` (opt-in; ``"f32"`` is the default and unchanged): ``"bf16x3"`` runs every GEMM — extractor layers 1 - 6, the projection,
    q | k | v, ``out_proj`` and the feed-forward's two — as x w ~ hi hi + hi lo + lo hi on bf16 MFMAs with fp32 accumulation (hi = bf16(x),
    lo = bf16(x - hi)); ``"bf16x3a"`` is that with the attention's two products in the same form too.  Everything else — statistics, layer 0,
    LayerNorms, GELUs, the positional conv, softmax, biases, the residual stream — stays fp32; outputs stay within 2e-4 of max|y| of the
    float64 restatement.  Keyword or ``set_precision``; kept by copies, pickles and ``load_state_dict``, not part of the ``state_dict``.

    ``config``: a mapping with the keys of the model's ``config.json`` (missing keys: the large model's).  Not built, refused at
    construction: group-norm extractors and post-LN encoders (HuBERT-base), WavLM's gated relative position bias (``features.WavLM`` reads
    those configurations), adapters, head sizes other than 64; ``masked_spec_embed`` is held for ``strict=True`` and never used (spec-augment
    is a training device)."""

    _PREFIX = "hificar_hubert"
    _NAME = "HuBERT"
    _PRECISIONS = _native.HUBERT_PRECISIONS
    _check_config = staticmethod(_native.check_hubert_config)
    sampling_rate = 16000

    def __init__(self, config=None, normalize=True, norm_eps=1e-7, precision="f32"):
        super().__init__()
        self.precision = self._check_precision(precision)
        c = self._check_config(dict(config or {}))
        self.config = c
        self.normalize, self.norm_eps = bool(normalize), float(norm_eps)
        C, H, I = c["conv_dim"][0], c["hidden_size"], c["intermediate_size"]
        LN, Lin = torch.nn.LayerNorm, torch.nn.Linear
        if c["mask_time_prob"] > 0.0 or c["mask_feature_prob"] > 0.0:  # (as the library decides; never read)
            self.masked_spec_embed = torch.nn.Parameter(torch.rand(H))
        self.feature_extractor = _Holder(conv_layers=torch.nn.ModuleList(
            _Holder(conv=torch.nn.Conv1d(1 if i == 0 else C, C, k, stride=s, bias=bool(c["conv_bias"])), layer_norm=LN(C))
            for i, (k, s) in enumerate(zip(_native.HUBERT_CONV_KERNEL, _native.HUBERT_CONV_STRIDE))))
        self.feature_projection = _Holder(layer_norm=LN(C, eps=c["layer_norm_eps"]), projection=Lin(C, H))
        # the positional conv under the names torch.nn.utils.parametrizations.weight_norm(conv, dim=2) gives it (original0: g, original1: v),
        # as plain holders: a parametrized module cannot be pickled
        K, G = _native.HUBERT_POS_TAPS, H // _native.HUBERT_POS_GROUPS
        wn = _Holder()
        bound = (G * K) ** -0.5
        wn.original1 = torch.nn.Parameter(torch.empty(H, G, K).uniform_(-bound, bound))
        wn.original0 = torch.nn.Parameter(wn.original1.detach().pow(2).sum((0, 1), keepdim=True).sqrt())
        wn._parameters = {k: wn._parameters[k] for k in ("original0", "original1")}  # (the library's order)
        pos = _Holder()
        pos.bias = torch.nn.Parameter(torch.empty(H).uniform_(-bound, bound))
        pos.parametrizations = _Holder(weight=wn)
        self.encoder = _Holder(pos_conv_embed=_Holder(conv=pos), layer_norm=LN(H, eps=c["layer_norm_eps"]), layers=torch.nn.ModuleList(
            _Holder(attention=_Holder(k_proj=Lin(H, H), v_proj=Lin(H, H), q_proj=Lin(H, H), out_proj=Lin(H, H)), layer_norm=LN(H, eps=c["layer_norm_eps"]),
                    feed_forward=_Holder(intermediate_dense=Lin(H, I), output_dense=Lin(I, H)), final_layer_norm=LN(H, eps=c["layer_norm_eps"]))
            for _ in range(c["num_hidden_layers"])))
        self._extend(c)
        self._params = {"in_channels": 1, "out_channels": H}
        self._init_native()
        self.eval()

    def _extend(self, c):
        """Parameter holders a subclass adds to the hierarchy, before the native state is set up."""

    @classmethod
    def _check_precision(cls, precision):
        if not isinstance(precision, str) or precision not in cls._PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(cls._PRECISIONS)}")
        return precision

    def set_precision(self, precision):
        """Switch the encoder's arithmetic: ``"f32"``, ``"bf16x3"`` or ``"bf16x3a"`` (the class docstring).  The native handle is dropped, so
        the next forward rebuilds it from the module's parameters and packs the weights for that arithmetic (hificar_hubert_set_precision
        between create and finalize); back on ``"f32"`` the model gives the bytes it gave before."""
        precision = self._check_precision(precision)
        if precision != self.precision:
            self.precision = precision
            self._invalidate()

    def __setstate__(self, state):
        state.setdefault("precision", "f32")  # (a pickle from before the keyword)
        super().__setstate__(state)

    def _finalize_handle(self, handle):
        self._call("_set_precision", handle, _native.HUBERT_PRECISIONS[self.precision])
        self._call("_finalize", handle)

    # ------------------------------------------------------------------ what NativeFeatureModel asks of a model
    def _device(self):
        return self.encoder.layer_norm.weight.device

    def _make_config(self):
        return _native.make_hubert_config(self.config, self.normalize, self.norm_eps)

    def _batch_norms(self):
        return []

    def native_state(self):
        """{name as hificar_hubert_set_weight takes it: fp32 CPU tensor}: the state_dict without masked_spec_embed, the positional conv's
        weight norm under its old names."""
        out = {}
        for k, v in self.state_dict().items():
            if k == "masked_spec_embed":
                continue
            k = k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v")
            out[k] = v.detach().float().cpu().contiguous()
        return out

    def load_state_dict(self, state_dict, strict=True, **kw):
        """``HubertModel``'s keys; ``encoder.pos_conv_embed.conv.weight_g`` / ``weight_v`` are taken for the parametrized names."""
        p = "encoder.pos_conv_embed.conv."
        sd = {(p + _WEIGHT_NORM_OLD[k[len(p):]] if k.startswith(p) and k[len(p):] in _WEIGHT_NORM_OLD else k): v for k, v in state_dict.items()}
        return super().load_state_dict(sd, strict=strict, **kw)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError(f"{self._NAME}: training (dropout, spec-augment, layerdrop, a backward pass) is not built; the module is inference-only")
        return super().train(False)

    @classmethod
    def from_pretrained(cls, directory, normalize=True, norm_eps=1e-7, precision="f32"):
        """A model from a directory in the ``transformers`` layout: ``config.json`` and ``model.safetensors`` (when ``safetensors`` imports) or
        ``pytorch_model.bin``.  fairseq and s3prl checkpoints are refused: neither layout could be checked against its package here."""
        import json
        import os

        with open(os.path.join(directory, "config.json")) as f:
            config = json.load(f)
        model = cls(config, normalize=normalize, norm_eps=norm_eps, precision=precision)
        st_path, bin_path = os.path.join(directory, "model.safetensors"), os.path.join(directory, "pytorch_model.bin")
        sd = None
        if os.path.exists(st_path):
            try:
                from safetensors.torch import load_file
            except ImportError:
                load_file = None
            if load_file is not None:
                sd = load_file(st_path)
        if sd is None:
            if not os.path.exists(bin_path):
                raise FileNotFoundError(f"{directory}: neither pytorch_model.bin nor a readable model.safetensors")
            sd = torch.load(bin_path, map_location="cpu", weights_only=True)
        if not isinstance(sd, dict) or any(k in sd for k in ("model", "cfg", "args", "Upstream", "Config")) or \
                any(isinstance(k, str) and (".self_attn." in k or k.startswith("w2v_encoder.")) for k in sd):
            raise NotImplementedError(f"{directory}: a fairseq / s3prl checkpoint layout; only the transformers layout (HubertModel's keys) is read")
        model.load_state_dict(sd, strict=True)
        return model

    @staticmethod
    def frames(length):
        """Frames of an utterance of ``length`` samples: ``(length - 400) // 320 + 1``; ValueError under 400 samples."""
        return _native.hubert_frames(length)

    def debug_tap(self, name, dst):
        """Test aid (hificar_hubert_debug_tap): the following forwards copy the named intermediate into ``dst`` (a float32 device tensor).
        ``"extractor.0"`` exists on an ``"f32"`` model only (the other arithmetics hold layer 0's rows as split bf16 rows): refused by name."""
        handle = self._native_handle()
        self._call("_debug_tap", handle, name.encode() if name is not None else None, None if dst is None else dst.data_ptr(),
                   0 if dst is None else dst.numel())

    def workspace_bytes(self, B, L):
        """Bytes of device scratch a forward of B utterances of at most L samples takes (hificar_hubert_workspace_bytes; needs the handle)."""
        return int(self._fn("_workspace_bytes")(self._native_handle(), B, L))

    def forward(self, wav, lengths=None, layer=-1):
        """wav: (B, L) or (L,) float tensor on the device; lengths: B sample counts in 400 .. L, or None (every utterance has L); layer: -1 or
        0 .. N - 1.  Returns (feats (B, hidden_size, Tmax) float32, frames (B,) int32 on the device)."""
        name = self._NAME
        if not isinstance(wav, torch.Tensor) or wav.device.type != "cuda":
            raise RuntimeError(f"{name} needs a CUDA/HIP tensor; there is no CPU fallback")
        if wav.requires_grad:
            raise RuntimeError(f"{name}: wav requires grad, and no backward through the encoder is built (detach it)")
        if wav.dim() not in (1, 2) or not wav.is_floating_point():
            raise RuntimeError(f"{name}: expected a (B, L) or (L,) float tensor, got {tuple(wav.shape)} {wav.dtype}")
        n_layers = self.config["num_hidden_layers"]
        if isinstance(layer, bool) or not isinstance(layer, int) or not -1 <= layer < n_layers:
            raise ValueError(f"{name}: layer must be -1 or in 0 .. {n_layers - 1}, got {layer!r}")
        y = wav.reshape(1, -1) if wav.dim() == 1 else wav
        y = y.detach().to(torch.float32).contiguous()
        B, L = y.shape
        if B < 1:
            raise RuntimeError(f"{name}: empty batch {tuple(wav.shape)}")
        T = self.frames(L)
        lens = (None, None)
        keep = None
        if lengths is not None:
            host = lengths.detach().to("cpu", torch.int32) if isinstance(lengths, torch.Tensor) else torch.as_tensor(lengths, dtype=torch.int32)
            host = host.reshape(-1).contiguous()
            if host.numel() != B:
                raise RuntimeError(f"{name}: lengths has {host.numel()} entries for a batch of {B}")
            if int(host.max()) > L:
                raise RuntimeError(f"{name}: lengths must lie in [{_native.HUBERT_MIN_SAMPLES}, {L}]")
            self.frames(int(host.min()))
            keep = (host, host.to(y.device))
            lens = (keep[1].data_ptr(), keep[0].data_ptr())
            frames = torch.div(keep[1] - 400, 320, rounding_mode="floor").to(torch.int32) + 1
        else:
            frames = torch.full((B,), T, dtype=torch.int32, device=y.device)
        handle = self._native_handle()
        if y.device != self._device():
            raise RuntimeError(f"{name}: input on {y.device}, parameters on {self._device()}")
        with torch.cuda.device(y.device):
            n = int(self._fn("_workspace_bytes")(handle, B, L))
            if n == 0:
                raise RuntimeError(f"{name}: B={B}, L={L} out of range (B <= 65535, B frames max(3 hidden, intermediate) < 2^31)")
            ws_ptr, ws_bytes = scratch(self, "_workspace_buf", n, self._device)
            out = torch.empty((B, self.config["hidden_size"], T), dtype=torch.float32, device=y.device)
            self._call("_forward", handle, y.data_ptr(), lens[0], lens[1], out.data_ptr(), B, L, layer, ws_ptr, ws_bytes, current_stream())
        del keep
        return out, frames

    def forward_lowrate(self, *a, **kw):
        raise NotImplementedError(f"{self._NAME} has no low-rate front end: it IS the front end (its output goes into a model's forward_lowrate)")


class WavLM(HuBERT):
    """The WavLM encoder of the "large" family (``wavlm-large``'s architecture: HuBERT-large's extractor, projection, positional conv,
    stable-layer-norm layers and final LayerNorm, plus the gated relative position bias in every layer's attention), the speech model whose
    ``hidden_states[9]`` the reference's ``egs/ema/voc1/local/linear_inference.py`` feeds to a fitted linear regression.  ``state_dict()`` has
    the keys and shapes of the ``transformers`` library's ``WavLMModel`` in its order and loads with ``strict=True``.  Same call shape,
    ``from_pretrained``, pickling, ``debug_tap`` and ``workspace_bytes`` as ``HuBERT``:

        feats, frames = wavlm(wav, lengths=samples, layer=9)            # (B, 1024, Tmax) at 50 Hz; layers 9 .. 23 are not run
        ema = head(feats, frames)                                       # features.LinearHead

    The attention's scores are ``Q K / sqrt(d) + gate[b, h, q] * rel_attn_embed[bucket(k - q), h]``: layer 0 owns the embedding
    (``num_buckets`` rows), every layer its own gate (``gru_rel_pos_linear``, ``gru_rel_pos_const``) computed from the layer's attention input.
    The bucket of every distance is computed here, once, with torch's float32 operations (``_native.wavlm_bucket_of_distance``) and handed to
    ``hificar_hubert_set_rel_bias``; the (heads, T, T) bias the library materialises never exists on the device.  The debug tap ``"gate.<l>"``
    is (B, heads, Tmax): the gates layer l used.

    ``precision``: ``"f32"`` (default) or ``"bf16x3"`` (``HuBERT``'s; the gates are the same bits in both).  ``"bf16x3a"`` is refused: the
    bf16 attention kernel has no bias term.  ``config``: missing keys take the large model's values, ``num_buckets`` 320 and
    ``max_bucket_distance`` 800.  Not built, refused at construction: group-norm extractors and post-LN encoders (``wavlm-base``,
    ``wavlm-base-plus``), adapters, head sizes other than 64.  s3prl's ``hidden_states[k]`` is, by reading its code, the stream in front of
    layer k, the same as the library's and as ``layer=k`` here; s3prl is not on hand, so this is unverified."""

    _NAME = "WavLM"
    _PRECISIONS = _native.WAVLM_PRECISIONS
    _check_config = staticmethod(_native.check_wavlm_config)

    @classmethod
    def _check_precision(cls, precision):
        if precision == "bf16x3a":
            raise ValueError("WavLM: precision='bf16x3a' is not built: the bf16 attention kernel has no relative position bias "
                             f"(choose from {sorted(cls._PRECISIONS)})")
        return super()._check_precision(precision)

    def _extend(self, c):
        heads = c["num_attention_heads"]
        for l, layer in enumerate(self.encoder.layers):
            att = layer.attention
            att.gru_rel_pos_linear = torch.nn.Linear(_native.HUBERT_HEAD_DIM, 8)
            if l == 0:
                att.rel_attn_embed = torch.nn.Embedding(c["num_buckets"], heads)
            att.gru_rel_pos_const = torch.nn.Parameter(torch.ones(1, heads, 1, 1))

    @staticmethod
    def _is_rel_bias(key):
        return "gru_rel_pos" in key or key.endswith("rel_attn_embed.weight")

    def native_state(self):
        """``HuBERT.native_state`` without the relative bias's tensors: hificar_hubert_set_weight takes those only once
        hificar_hubert_set_rel_bias was called (``rel_bias_state``, ``_finalize_handle``)."""
        return {k: v for k, v in super().native_state().items() if not self._is_rel_bias(k)}

    def rel_bias_state(self):
        """{name: fp32 CPU tensor} of ``rel_attn_embed`` and every layer's ``gru_rel_pos_linear`` / ``gru_rel_pos_const``."""
        return {k: v for k, v in super().native_state().items() if self._is_rel_bias(k)}

    def _finalize_handle(self, handle):
        c = self.config
        self._call("_set_precision", handle, _native.WAVLM_PRECISIONS[self.precision])
        table = _native.wavlm_bucket_of_distance(c["num_buckets"], c["max_bucket_distance"])
        self._call("_set_rel_bias", handle, c["num_buckets"], c["max_bucket_distance"], table.data_ptr())
        for name, t in self.rel_bias_state().items():
            shape = (ctypes.c_int64 * t.dim())(*t.shape)
            self._call("_set_weight", handle, name.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim())
        self._call("_finalize", handle)


def ssl_encoder_from_pretrained(directory, **kw):
    """``HuBERT.from_pretrained`` or ``WavLM.from_pretrained`` by the ``model_type`` of ``directory``'s ``config.json`` (absent: HuBERT, unless
    the configuration has WavLM's ``num_buckets``).  Keywords as theirs."""
    return ssl_encoder_class(directory).from_pretrained(directory, **kw)


def ssl_encoder_class(directory):
    """The class ``ssl_encoder_from_pretrained`` loads ``directory`` with, from its ``config.json`` alone."""
    import json
    import os

    with open(os.path.join(directory, "config.json")) as f:
        config = json.load(f)
    model_type = str(config.get("model_type", "wavlm" if "num_buckets" in config else "hubert")).lower()
    if model_type not in ("hubert", "wavlm"):
        raise NotImplementedError(f"{directory}: model_type {model_type!r}: only 'hubert' (features.HuBERT) and 'wavlm' (features.WavLM) are built")
    return WavLM if model_type == "wavlm" else HuBERT


class LinearHead(NativeOwner, torch.nn.Module):
    """``y = coef x + intercept`` over device features: (B, H, T) -> (B, out, T), the fitted linear regression the reference's
    ``egs/ema/voc1/local/linear_inference.py`` applies to ``hidden_states[9]`` of ``wavlm_large``.  It runs in ``libhificar.so`` as the one-tap
    GEMM every ``Linear`` of this package is (``hificar_linear_*`` of include/hificar.h; exact fp32 only — the regression is tiny): every
    utterance is computed as if alone, bit for bit, and rows from an utterance's own frame count on are exact zeros.  No CPU fallback, no
    backward.

        head = LinearHead.load("linear.joblib").to("cuda")
        feats, frames = wavlm(wav, lengths=samples, layer=9)
        ema = head(feats, frames)                                       # (B, out, Tmax)

    ``coef``: (out, H), ``intercept``: (out,) — sklearn's ``coef_`` / ``intercept_`` (a 1-D ``coef_`` is one output)."""

    _DESTROY = "hificar_linear_destroy"
    _ENGINE = "hificar_linear_engine"
    _NATIVE = {"_handle": None, "_handle_key": None, "_workspace_buf": None}

    def __init__(self, coef, intercept):
        super().__init__()
        coef = torch.from_numpy(np.array(coef, dtype=np.float32))  # (copies: a fitted model's arrays may be read-only)
        coef = coef.reshape(1, -1) if coef.dim() == 1 else coef
        intercept = torch.from_numpy(np.array(intercept, dtype=np.float32)).reshape(-1)
        if coef.dim() != 2 or intercept.numel() != coef.shape[0]:
            raise ValueError(f"LinearHead: coef {tuple(coef.shape)} and intercept {tuple(intercept.shape)} do not make out x in and out")
        if not 1 <= coef.shape[1] <= _native.LINEAR_MAX_IN or not 1 <= coef.shape[0] <= _native.LINEAR_MAX_OUT:
            raise ValueError(f"LinearHead: {coef.shape[1]} -> {coef.shape[0]} features out of range (1 .. {_native.LINEAR_MAX_IN} in, "
                             f"1 .. {_native.LINEAR_MAX_OUT} out)")
        self.register_buffer("coef", coef.contiguous().clone())
        self.register_buffer("intercept", intercept.contiguous().clone())
        self._reset_native()

    in_features = property(lambda self: self.coef.shape[1])
    out_features = property(lambda self: self.coef.shape[0])

    @classmethod
    def load(cls, path):
        """A head from a ``.joblib`` file — a fitted sklearn ``LinearRegression`` or ``Ridge``, anything with ``coef_`` and ``intercept_``
        (``joblib`` is imported only here) — or from an ``.npz`` with ``coef`` and ``intercept``."""
        if str(path).endswith(".npz"):
            with np.load(path) as z:
                if "coef" not in z.files or "intercept" not in z.files:
                    raise ValueError(f"{path}: an .npz head holds 'coef' and 'intercept', this one has {sorted(z.files)}")
                return cls(z["coef"], z["intercept"])
        if not str(path).endswith(".joblib"):
            raise ValueError(f"{path}: a linear head is a .joblib (a fitted sklearn LinearRegression / Ridge) or an .npz with coef / intercept")
        try:
            import joblib
        except ImportError:
            raise RuntimeError(f"{path}: reading a .joblib head needs the joblib package, which does not import here; save coef_ / intercept_ "
                               "as an .npz with 'coef' and 'intercept' instead") from None
        reg = joblib.load(path)
        if not hasattr(reg, "coef_") or not hasattr(reg, "intercept_"):
            raise ValueError(f"{path}: {type(reg).__name__} has no coef_ / intercept_ (a fitted LinearRegression or Ridge is read)")
        coef = np.asarray(reg.coef_)
        coef = coef.reshape(1, -1) if coef.ndim == 1 else coef
        return cls(coef, np.broadcast_to(np.asarray(reg.intercept_, dtype=np.float64).reshape(-1), (coef.shape[0],)))

    def _native_handle(self):
        key = (self.coef.device, self.coef.data_ptr(), self.coef._version, self.intercept.data_ptr(), self.intercept._version)
        if self._handle is not None and self._handle_key != key:
            self._invalidate()
        if self._handle is None:
            self._lib = _native.load_library()
            coef, intercept = self.coef.detach().cpu().contiguous(), self.intercept.detach().cpu().contiguous()
            handle = ctypes.c_void_p()
            with torch.cuda.device(self.coef.device):
                _native.check(self._lib.hificar_linear_create(coef.shape[1], coef.shape[0], coef.data_ptr(), intercept.data_ptr(), ctypes.byref(handle)),
                              "hificar_linear_create")
            self._handle, self._handle_key = handle, key
        return self._handle

    def forward(self, feats, lengths=None):
        """feats: (B, H, T) float tensor on the device; lengths: B frame counts in 0 .. T (a device int32 tensor — ``frames`` as ``WavLM``
        returns it — is used as it is; anything else is copied), or None (every sequence has T).  Returns (B, out, T) float32."""
        if not isinstance(feats, torch.Tensor) or feats.device.type != "cuda":
            raise RuntimeError("LinearHead needs a CUDA/HIP tensor; there is no CPU fallback")
        if feats.requires_grad:
            raise RuntimeError("LinearHead: feats requires grad, and no backward is built (detach it)")
        if feats.dim() != 3 or feats.shape[1] != self.in_features or not feats.is_floating_point():
            raise RuntimeError(f"LinearHead: expected a (B, {self.in_features}, T) float tensor, got {tuple(feats.shape)} {feats.dtype}")
        if feats.device != self.coef.device:
            raise RuntimeError(f"LinearHead: input on {feats.device}, coefficients on {self.coef.device}")
        x = feats.detach().to(torch.float32).contiguous()
        B, _, T = x.shape
        if B < 1 or T < 1:
            raise RuntimeError(f"LinearHead: empty batch {tuple(feats.shape)}")
        lens = None
        if lengths is not None:
            lens = lengths if isinstance(lengths, torch.Tensor) else torch.as_tensor(lengths)
            lens = lens.detach().reshape(-1).to(x.device, torch.int32).contiguous()
            if lens.numel() != B:
                raise RuntimeError(f"LinearHead: lengths has {lens.numel()} entries for a batch of {B}")
        handle = self._native_handle()
        lib = self._lib
        with torch.cuda.device(x.device):
            n = int(lib.hificar_linear_workspace_bytes(handle, B, T))
            if n == 0:
                raise RuntimeError(f"LinearHead: B={B}, T={T} out of range (B <= 65535, B T max(in, out) < 2^31)")
            ws_ptr, ws_bytes = scratch(self, "_workspace_buf", n, x.device)
            out = torch.empty((B, self.out_features, T), dtype=torch.float32, device=x.device)
            rc = lib.hificar_linear_forward(handle, x.data_ptr(), None if lens is None else lens.data_ptr(), out.data_ptr(), B, T, ws_ptr, ws_bytes,
                                            current_stream())
        _native.check(rc, "hificar_linear_forward")
        del lens
        return out
