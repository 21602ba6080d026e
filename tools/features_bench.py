#!/usr/bin/env python3
"""Device time of the speech features (articulatory_amd.features) at a workload size: B utterances of --seconds at 16 kHz.

Three legs, one JSON line each (appended to --out):

  features     MFCC (13 / 40 / 320, hop 80) and LogMel (1024 / 256 / 80) in windows of at least --window seconds, alternated
               MFCC / LogMel / MFCC / LogMel in one process: the two windows of a feature run on unchanged code, their difference is the
               spread a reader should hold any other difference against.  Device time from events around blocks of calls.
  predict_ema  what predict_ema --from-wav does per batch on the device — MFCC, then BiGRU.forward_lowrate(zscore=True) — against the
               forward_lowrate alone on features already there, alternated the same way: the front end's share of speech -> EMA.
  cpu          the float64 chain (torch.stft -> filterbank -> power_to_db -> DCT, utterance by utterance, as the reference calls
               librosa) on 1 and 16 CPU threads, wall clock.  NOT librosa: the only stand-in available where librosa is not installed,
               labelled as such wherever the number is quoted.

Operations and bytes printed beside the times are computed from the shapes (the DFT GEMM's 2 M N 2 nf, the buffers each pass reads and
writes), not measured.
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from articulatory_amd import _native  # noqa: E402
from articulatory_amd.features import MFCC, LogMel  # noqa: E402
from articulatory_amd.models import BiGRU  # noqa: E402
from articulatory_amd.utils.mel import mel_filterbank  # noqa: E402
from articulatory_amd.utils.synth import synth_bigru_state_dict  # noqa: E402

SR = 16000
BIGRU = dict(in_channels=13, hidden_size=256, out_channels=12, use_tanh=True)  # the published width on MFCC inputs


def window(fn, seconds, limit):
    """Mean device milliseconds per call over a window of at least `seconds` (events around blocks of calls)."""
    total_ms, calls, n = 0.0, 0, 1
    while total_ms < seconds * 1e3:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms / n > limit * 1e3:
            raise SystemExit(f"a call took {ms / n:.0f} ms, over the limit of {limit} s")
        total_ms += ms
        calls += n
        n = min(n * 2, 16)
    return total_ms / calls


def alternated(a, b, seconds, limit):
    for _ in range(3):
        a()
        b()
    torch.cuda.synchronize()
    a1 = window(a, seconds, limit)
    b1 = window(b, seconds, limit)
    a2 = window(a, seconds, limit)
    b2 = window(b, seconds, limit)
    return [round(a1, 4), round(a2, 4)], [round(b1, 4), round(b2, 4)]


def kernel_profile(f, fn):
    """{kernel: device ms} of one call, from the library's event profile."""
    lib, eng = f._lib, f.engine()
    _native.check(lib.hificar_profile_begin(eng), "hificar_profile_begin")
    fn()
    return {r["name"]: round(r["total_ms"], 4) for r in _native.profile_rows(lib, eng, 64)[0]}


def counted(f, B, L):
    """GFLOP of the DFT GEMM and MB the passes move, from the shapes."""
    N, nf, nm, C = f.fft_size, f.fft_size // 2 + 1, f.melmat.shape[0], f.channels
    M = B * (1 + L // f.hop_size)
    nfp = -(-nf // 32) * 32
    flop = 2.0 * M * N * 2 * nfp
    byts = 4.0 * (B * L + M * N) + 4.0 * (M * N + M * 2 * nfp) + 4.0 * (M * 2 * nf + M * nm) + 4.0 * (M * nm + M * C)
    return round(flop / 1e9, 2), round(byts / 1e6, 1)


def cpu_chain(wav, kind, threads):
    """Seconds of the float64 chain over the batch, one utterance at a time."""
    torch.set_num_threads(threads)
    if kind == "mfcc":
        n_fft, hop, nm = 320, 80, 40
    else:
        n_fft, hop, nm = 1024, 256, 80
    fb = torch.from_numpy(mel_filterbank(SR, n_fft, nm, 0.0, SR / 2).astype(np.float64))
    w = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    j, k = np.arange(13)[:, None], np.arange(nm)[None, :]
    dct = torch.from_numpy(np.sqrt(np.where(j == 0, 1.0, 2.0) / nm) * np.cos(np.pi * j * (2 * k + 1) / (2.0 * nm)))
    t0 = time.perf_counter()
    for y in wav:
        S = torch.stft(y, n_fft, hop_length=hop, window=w, center=True, pad_mode="reflect", return_complex=True)
        if kind == "mfcc":
            db = 10.0 * torch.log10(torch.clamp(fb @ (S.real ** 2 + S.imag ** 2), min=1e-10))
            out = dct @ torch.maximum(db, db.max() - 80.0)
        else:
            out = torch.log10(torch.clamp(fb @ S.abs(), min=1e-10))
    assert out.dtype == torch.float64
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--limit", type=float, default=5.0, help="seconds a single call may take")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("features_bench: no GPU visible; a device time is measured on the device or not at all")
    B, L = a.batch, int(a.seconds * SR)
    g = torch.Generator().manual_seed(0)
    wav_host = 0.1 * torch.randn((B, L), generator=g, dtype=torch.float64)
    wav = wav_host.float().cuda()
    lines = []

    mfcc, logmel = MFCC(sampling_rate=SR, hop_length=80), LogMel(SR)
    m_ms, l_ms = alternated(lambda: mfcc(wav), lambda: logmel(wav), a.window, a.limit)
    res = {"leg": "features", "B": B, "samples": L, "mfcc_hop80_ms": m_ms, "logmel_1024_256_ms": l_ms,
           "mfcc_spread": round(abs(m_ms[0] - m_ms[1]) / min(m_ms), 4), "logmel_spread": round(abs(l_ms[0] - l_ms[1]) / min(l_ms), 4)}
    for name, f in (("mfcc", mfcc), ("logmel", logmel)):
        res[name + "_dft_gflop"], res[name + "_mb_moved"] = counted(f, B, L)
        res[name + "_workspace_mb"] = round(int(f._lib.hificar_feat_workspace_bytes(f._handle, B, L)) / 1e6, 1)
        res[name + "_kernels_ms"] = kernel_profile(f, lambda: f(wav))
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)

    model = BiGRU(**BIGRU)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth_bigru_state_dict(BIGRU, seed=5101).items()}, strict=True)
    model = model.eval().cuda()
    lens = [L] * B
    frames = [mfcc.frames(L)] * B
    with torch.no_grad():
        feats, _ = mfcc(wav, lens)

        def from_wav():
            x, _ = mfcc(wav, lens)
            return model.forward_lowrate(x, lengths=frames, interp_factor=1, zscore=True)

        def from_feats():
            return model.forward_lowrate(feats, lengths=frames, interp_factor=1, zscore=True)

        w_ms, f_ms = alternated(from_wav, from_feats, a.window, a.limit)
    res = {"leg": "predict_ema", "B": B, "samples": L, "frames": frames[0], "bigru": BIGRU, "from_wav_ms": w_ms, "from_features_ms": f_ms,
           "front_end_ms": round(min(w_ms) - max(f_ms), 4), "front_end_share": round((min(w_ms) - max(f_ms)) / min(w_ms), 4)}
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)

    if not a.no_cpu:
        res = {"leg": "cpu", "what": "float64 torch.stft chain, utterance by utterance; a stand-in for librosa, NOT librosa", "B": B, "samples": L}
        for threads in (1, 16):
            for kind in ("mfcc", "logmel"):
                cpu_chain(wav_host[:2], kind, threads)
                res[f"{kind}_{threads}thr_s"] = round(cpu_chain(wav_host, kind, threads), 3)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
