"""Float64 restatement of the low-rate front end (the reference's egs/ema/voc1/local/predict_ema.py:83-101) for the tests, written from the
definitions (not from torch's or scipy's text):

    interp(x, f)   a sequence of l frames becomes f l:  src = max(0, (t + 0.5) / f - 0.5), i0 = floor(src), i1 = min(i0 + 1, l - 1),
                   lam = src - i0,  y[t] = (1 - lam) x[i0] + lam x[i1]      (F.interpolate(size=f l, mode='linear', align_corners=False))
    zscore(x)      (x - mean) / std over ALL C x l elements of the utterance, population std      (scipy.stats.zscore(axis=None))
    front_end      zscore first, then interp; in a padded batch every utterance by its own length, frames past f lengths[b] zero

``forward_lowrate(oracle, ...)`` composes it with ``BiGRUOracle`` / ``TransformerOracle`` (tests/bigru_oracle.py, tests/transformer_oracle.py),
which run every utterance of a ragged batch alone.  Test infrastructure only: no file of the package imports it.
"""

import numpy as np
import torch


def source_index(t, f, l):
    """(i0, i1, lam) of output frames ``t`` (an integer array) for ``l`` low-rate frames at factor ``f``; src is formed in exact integer
    arithmetic, (2 t + 1 - f) / (2 f), so lam is the correctly rounded fraction."""
    t = np.asarray(t, dtype=np.int64)
    num = np.maximum(2 * t + 1 - f, 0)
    i0 = np.minimum(num // (2 * f), l - 1)
    lam = (num % (2 * f)).astype(np.float64) / (2 * f)
    i1 = np.minimum(i0 + 1, l - 1)
    lam = np.where(i1 == i0, 0.0, lam)  # clamped at the last frame: the frame itself, bit for bit (l = 1 repeats its frame)
    return i0, i1, lam


def interp(x, f, dtype=np.float64, fused=False):
    """x (..., l) -> (..., f l) along the last axis.  ``fused`` (float32 only): the sum evaluated as torch's CPU kernel evaluates it,
    fma(1 - lam, x[i0], round(lam x[i1])) — the product and the sum formed in float64, where the product is exact, and rounded once."""
    x = np.asarray(x, dtype=dtype)
    l = x.shape[-1]
    if l == 0:
        return np.zeros(x.shape[:-1] + (0,), dtype=dtype)
    i0, i1, lam = source_index(np.arange(f * l), f, l)
    lam = lam.astype(dtype)
    if fused:
        assert dtype == np.float32
        tail = (lam * x[..., i1]).astype(np.float32).astype(np.float64)
        return ((1 - lam).astype(np.float64) * x[..., i0].astype(np.float64) + tail).astype(np.float32)
    return (1 - lam) * x[..., i0] + lam * x[..., i1]


def zscore(x):
    """One utterance (C, l): mean and population standard deviation over all its elements, in float64, two passes."""
    x = np.asarray(x, dtype=np.float64)
    mu = x.sum() / x.size
    sd = np.sqrt(((x - mu) ** 2).sum() / x.size)
    return (x - mu) / sd


def front_end(x, lengths=None, interp_factor=1, zscore_on=False):
    """x (B, C, Tl) -> float64 (B, C, f Tl): every utterance by its own low-rate length (None: all Tl), zeros past f lengths[b]; padded
    frames of x are never read."""
    x = np.asarray(x)
    B, C, Tl = x.shape
    lengths = [Tl] * B if lengths is None else [int(n) for n in lengths]
    out = np.zeros((B, C, interp_factor * Tl), dtype=np.float64)
    for b, l in enumerate(lengths):
        if l == 0:
            continue
        u = np.asarray(x[b, :, :l], dtype=np.float64)
        if zscore_on:
            u = zscore(u)
        out[b, :, :interp_factor * l] = interp(u, interp_factor)
    return out


def forward_lowrate(oracle, x, lengths=None, interp_factor=1, zscore_on=False):
    """predict_ema.py:83-101 on a batch: the front end, then the model's oracle on every utterance alone -> torch (B, out, f Tl)."""
    x = np.asarray(x)
    feats = front_end(x, lengths, interp_factor, zscore_on)
    hi = None if lengths is None else [interp_factor * int(n) for n in lengths]
    return oracle.forward(torch.from_numpy(feats), lengths=hi)
