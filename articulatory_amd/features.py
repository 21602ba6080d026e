"""Speech features on the device: ``MFCC`` — what the reference's ``egs/ema/voc1/local/predict_ema.py:32-33`` takes from
``librosa.feature.mfcc`` in front of its MFCC inversion models — and ``LogMel`` — the log-mel filterbank of
``articulatory/bin/preprocess.py:26-82``, the 80-channel input ``BiGRU()`` defaults to.  Both are ``torch.nn.Module``s without parameters over
one native handle (``hificar_feat_*`` of include/hificar.h): waveforms on the device in, features on the device out, ragged batches with
every utterance computed as if alone.  MI355X-native; there is no CPU fallback and no backward.

The arithmetic restates librosa 0.8.1's published algorithm (``stft(center=True, pad_mode="reflect")``, the Slaney filterbank of
``utils.mel``, ``power_to_db``, ``scipy.fftpack.dct(type=2, norm="ortho")``); librosa is not a dependency and parity with it is not pinned.
The z-score of ``wav2mfcc`` is not part of ``MFCC``: ``model.forward_lowrate(feats, lengths=frames, interp_factor=1, zscore=True)`` does it.
"""

import ctypes

import numpy as np
import torch

from . import _native
from .utils.mel import mel_filterbank


class _SpeechFeature(torch.nn.Module):
    """What ``MFCC`` and ``LogMel`` share: the native handle (made on first use, never shared by copies or pickles), the grow-only workspace
    and the call."""

    _NAME = None

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
        self._lib = self._handle = self._handle_dev = self._workspace_buf = None

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

    def _invalidate(self):
        handle, lib = self.__dict__.get("_handle"), self.__dict__.get("_lib")
        self.__dict__["_handle"] = None
        self.__dict__["_workspace_buf"] = None
        if handle is not None and lib is not None:
            lib.hificar_feat_destroy(handle)

    def __del__(self):
        try:
            self._invalidate()
        except Exception:
            pass

    def __getstate__(self):  # copies and pickles never share a native handle
        state = self.__dict__.copy()
        state["_handle"] = state["_lib"] = state["_handle_dev"] = state["_workspace_buf"] = None
        return state

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
            ws = self._workspace_buf
            if ws is None or ws.device != y.device or ws.numel() < n + 256:
                # work already enqueued on the old buffer keeps it alive through the caching allocator's stream ordering
                ws = torch.empty(int((n + 256) * 1.25) if ws is not None else n + 256, dtype=torch.uint8, device=y.device)
                self._workspace_buf = ws
            off = (-ws.data_ptr()) % 256
            out = torch.empty((B, self.channels, T), dtype=torch.float32, device=y.device)
            frames = torch.empty((B,), dtype=torch.int32, device=y.device)
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc = lib.hificar_feat_forward(handle, y.data_ptr(), lens[0], lens[1], out.data_ptr(), frames.data_ptr(), B, L, ws.data_ptr() + off,
                                          ws.numel() - off, stream)
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
