"""The speech features of ``articulatory_amd.features`` restated in numpy: MFCC as librosa 0.8.1's ``feature.mfcc`` computes it for the
reference's ``wav2mfcc`` (egs/ema/voc1/local/predict_ema.py:32-33: melspectrogram(power=2) -> power_to_db -> scipy.fftpack.dct(type=2,
norm="ortho")[:n_mfcc]) and the log-mel filterbank of ``articulatory/bin/preprocess.py:58-82``.  librosa reads float64 wavs and keeps that
precision, so the reference's arithmetic is ``dtype=np.float64``; ``dtype=np.float32`` is the same statement in the device's number format
(numpy's summation order, not the MFMA tiles'), which the accuracy bars of the GPU tests are set from (tests/test_speech_features_host.py).

A restatement of the published algorithm, parity-unpinned: librosa is not installed where this runs.

Also here: the inputs both the host emulation and the GPU tests use, so that the bars are set on exactly what the GPU tests run.
"""

import numpy as np

from articulatory_amd.utils.mel import mel_filterbank


def frame_matrix(y, n_fft, hop, dtype):
    """(T, n_fft) frames of ``librosa.stft(center=True, pad_mode="reflect")``: T = 1 + len(y) // hop."""
    y = np.asarray(y, dtype=dtype)
    if y.ndim != 1 or len(y) <= n_fft // 2:
        raise ValueError(f"reflect padding needs more than n_fft / 2 = {n_fft // 2} samples, got {y.shape}")
    yp = np.pad(y, n_fft // 2, mode="reflect")
    T = 1 + len(y) // hop
    return yp[np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]]


def dft_matrix(n_fft, win_length, dtype):
    """(n_fft, nf) cos and -sin matrices with the periodic Hann window of ``win_length``, centred in the frame, folded in: formed in
    float64, rounded once."""
    nf = n_fft // 2 + 1
    n = np.arange(n_fft)
    wn = n - (n_fft - win_length) // 2
    w = np.where((wn >= 0) & (wn < win_length), 0.5 - 0.5 * np.cos(2.0 * np.pi * wn / win_length), 0.0)
    ang = 2.0 * np.pi * ((n[:, None] * np.arange(nf)[None, :]) % n_fft) / n_fft
    return (w[:, None] * np.cos(ang)).astype(dtype), (-w[:, None] * np.sin(ang)).astype(dtype)


def power_spectrum(y, n_fft, hop, win_length, dtype):
    """(T, nf) re^2 + im^2."""
    A = frame_matrix(y, n_fft, hop, dtype)
    c, s = dft_matrix(n_fft, win_length, dtype)
    re, im = A @ c, A @ s
    return re * re + im * im


def dct_basis(n_mfcc, n_mels, dtype):
    """(n_mfcc, n_mels) rows of the orthonormal DCT-II (scipy.fftpack.dct(type=2, norm="ortho")), formed in float64, rounded once."""
    j, k = np.arange(n_mfcc)[:, None], np.arange(n_mels)[None, :]
    return (np.sqrt(np.where(j == 0, 1.0, 2.0) / n_mels) * np.cos(np.pi * j * (2 * k + 1) / (2.0 * n_mels))).astype(dtype)


def mfcc_db(y, sr=16000, n_mels=40, n_fft=320, hop_length=160, dtype=np.float64, amin=1e-10, top_db=80.0):
    """(n_mels, T) ``power_to_db(melspectrogram(y, power=2))``: the MFCC chain in front of the DCT."""
    fb = mel_filterbank(sr, n_fft, n_mels, 0.0, sr / 2).astype(dtype)  # float32 as librosa returns it
    mel = power_spectrum(y, n_fft, hop_length, n_fft, dtype) @ fb.T
    db = dtype(10.0) * np.log10(np.maximum(dtype(amin), mel))
    return np.maximum(db, db.max() - dtype(top_db)).T


def mfcc(y, sr=16000, n_mfcc=13, n_mels=40, n_fft=320, hop_length=160, dtype=np.float64):
    """(n_mfcc, T) ``librosa.feature.mfcc(y, sr, n_mfcc=, n_fft=, hop_length=, n_mels=)`` (0.8.1); no z-score."""
    return dct_basis(n_mfcc, n_mels, dtype) @ mfcc_db(y, sr, n_mels, n_fft, hop_length, dtype)


def zscore(x):
    """``scipy.stats.zscore(x, axis=None)`` in the array's own precision (population standard deviation)."""
    return (x - x.mean()) / x.std()


def logmel(y, sr, fft_size=1024, hop_size=256, win_length=None, num_mels=80, fmin=None, fmax=None, eps=1e-10, log_base=10.0, dtype=np.float64):
    """(num_mels, T): ``logmelfilterbank`` of preprocess.py:26-82, transposed (channels first, as the device returns it)."""
    fmin = 0 if fmin is None else fmin
    fmax = sr / 2 if fmax is None else fmax
    fb = mel_filterbank(sr, fft_size, num_mels, fmin, fmax).astype(dtype)
    spc = np.sqrt(power_spectrum(y, fft_size, hop_size, fft_size if win_length is None else win_length, dtype))
    mel = np.maximum(dtype(eps), spc @ fb.T)
    log = {None: np.log, 2.0: np.log2, 10.0: np.log10}[log_base]
    return log(mel).T


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
SR = 16000
MFCC_HOPS = (80, 160)
# 161: the shortest legal utterance (n_fft / 2 + 1; 3 frames at hop 80); 800 | 801: a hop boundary; 2560 | 2640: 32 | 33 frames at hop 80, the
# edge of the gather's and the output kernels' 32-frame tiles; 4000
MFCC_LENGTHS = (161, 800, 801, 2560, 2640, 4000)
# (label, keywords, lengths) of the log-mel cases
LOGMEL_CASES = (
    ("default", dict(), (3000, 8192)),
    ("small_ln", dict(fft_size=64, hop_size=16, win_length=48, num_mels=8, fmin=80, log_base=None), (3000, 8192)),
    ("small_log2", dict(fft_size=64, hop_size=16, win_length=48, num_mels=8, fmin=80, log_base=2.0), (3000, 8192)),
)


def voiced(rng, n, scale):
    """A harmonic tone with a slow envelope over a little noise: speech-like enough to fill every mel band."""
    t = np.arange(n) / SR
    f0 = rng.uniform(90.0, 220.0)
    y = sum(rng.uniform(0.2, 1.0) / h * np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 2 * np.pi)) for h in range(1, 30))
    y = y * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 0.02 * rng.standard_normal(n)
    return scale * y / np.abs(y).max()


def mfcc_batch():
    """(wav (6, 4000) float32 — NaN at and past every length —, lengths): utterance 3 is noise at 1e-4, utterance 4 runs at full scale
    (|y| reaches 1), utterance 5 holds a stretch of digital silence (whole frames of exact zeros: the floor at amin and the clamp at
    max - top_db are both active)."""
    rng = np.random.default_rng(20240611)
    wav = np.full((len(MFCC_LENGTHS), max(MFCC_LENGTHS)), np.nan, dtype=np.float32)
    for b, n in enumerate(MFCC_LENGTHS):
        if b == 3:
            y = 1e-4 * rng.standard_normal(n)
        elif b == 4:
            y = voiced(rng, n, 1.0)
        else:
            y = voiced(rng, n, rng.uniform(0.05, 0.4))
        if b == 5:
            y[1200:2400] = 0.0
        wav[b, :n] = y.astype(np.float32)
    return wav, np.asarray(MFCC_LENGTHS, dtype=np.int32)


def logmel_batch():
    """(wav (2, 8192) float32, NaN past the lengths, lengths (3000, 8192))."""
    rng = np.random.default_rng(20240612)
    lengths = LOGMEL_CASES[0][2]
    wav = np.full((len(lengths), max(lengths)), np.nan, dtype=np.float32)
    for b, n in enumerate(lengths):
        wav[b, :n] = voiced(rng, n, 0.3).astype(np.float32)
    return wav, np.asarray(lengths, dtype=np.int32)


# ------------------------------------------------------------------------------------------------ the bars
# Four times the float32 emulation's worst error over the inputs above (emulation_errors), rounded up to one significant digit; set before
# the first GPU run (tests/test_speech_features_host.py holds the table and checks it).
BAR_MFCC_REL = 6e-7   # MFCC relative to the utterance's max|c|          (emulation: 1.28e-7)
BAR_MFCC_Z = 2e-6     # z-scored MFCC, absolute                           (emulation: 4.80e-7)
BAR_LOGMEL = 4e-5     # log-mel, absolute, in the log's own base          (emulation: 8.36e-6)


def one_digit_up(x):
    """x rounded up to one significant digit."""
    e = np.floor(np.log10(x))
    return float(np.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e)


def emulation_errors():
    """The float32 restatement against the float64 one over exactly the inputs of the GPU tests: the worst error of
    (MFCC relative to the utterance's max|c|, z-scored MFCC, log-mel absolute)."""
    wav, lens = mfcc_batch()
    rel = zs = 0.0
    for hop in MFCC_HOPS:
        for b, n in enumerate(lens):
            c64 = mfcc(wav[b, :n], SR, hop_length=hop)
            c32 = mfcc(wav[b, :n], SR, hop_length=hop, dtype=np.float32)
            assert c32.dtype == np.float32
            rel = max(rel, float(np.abs(c32 - c64).max() / np.abs(c64).max()))
            zs = max(zs, float(np.abs(zscore(c32.astype(np.float64)) - zscore(c64)).max()))
    wav, lens = logmel_batch()
    lm = 0.0
    for _, kw, _ in LOGMEL_CASES:
        for b, n in enumerate(lens):
            a64 = logmel(wav[b, :n], SR, **kw)
            a32 = logmel(wav[b, :n], SR, dtype=np.float32, **kw)
            assert a32.dtype == np.float32
            lm = max(lm, float(np.abs(a32 - a64).max()))
    return rel, zs, lm
