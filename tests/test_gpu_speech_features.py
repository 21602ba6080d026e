"""``articulatory_amd.features`` (``MFCC``, ``LogMel``) and ``predict_ema --from-wav`` on a MI355X, against the float64 restatement
(tests/speech_features_oracle.py).  ``pytest -m gpu``.

Bars: tests/test_speech_features_host.py sets them from the float32 emulation over exactly these inputs (MFCC 6e-7 of the utterance's
max|c|, z-scored MFCC 2e-6, log-mel 4e-5); no element is excluded.  End to end the bar is the BiGRU eval path's own (2e-5 of max|y|,
tests/test_gpu_bigru.py).  Everything else is bitwise: an utterance alone and in the batch, two runs, NaN past the lengths over dirty
buffers, zeros from the utterance's own frame count on.
"""

import ctypes
import wave

import numpy as np
import pytest
import torch
import yaml

import speech_features_oracle as O
from conftest import rel_err
from articulatory_amd.bin import predict_ema as PE
from articulatory_amd.features import MFCC, LogMel
from articulatory_amd.models import BiGRU
from articulatory_amd.utils.synth import synth_bigru_state_dict

pytestmark = pytest.mark.gpu
TOL_BIGRU = 2e-5
BIGRU13 = (dict(in_channels=13, hidden_size=64, out_channels=12, use_tanh=True), 7102)  # the MFCC model of tests/test_gpu_predict_ema.py


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


@pytest.fixture(scope="module")
def mfcc_case():
    """The ragged batch and, per hop, the float64 MFCCs of every utterance: computed once, never written to."""
    wav, lens = O.mfcc_batch()
    ref = {hop: [O.mfcc(wav[b, :n], O.SR, hop_length=hop) for b, n in enumerate(lens)] for hop in O.MFCC_HOPS}
    return wav, lens, ref


@pytest.fixture(scope="module")
def bigru13():
    params, seed = BIGRU13
    sd = synth_bigru_state_dict(params, seed=seed)
    m = BiGRU(**params)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval().to("cuda:0"), sd, params


def run_native(f, wav, lens, fill):
    """hificar_feat_forward on buffers of the test's own: workspace and output filled with the byte ``fill`` first."""
    assert torch.cuda.is_available()
    x = dev(wav)
    B, L = x.shape
    handle, lib = f._native_handle(x.device), f._lib
    n = int(lib.hificar_feat_workspace_bytes(handle, B, L))
    assert n > 0
    ws = torch.full((n + 256,), fill, dtype=torch.uint8, device=x.device)
    off = (-ws.data_ptr()) % 256
    T = 1 + L // f.hop_size
    out = torch.full((B * f.channels * T * 4,), fill, dtype=torch.uint8, device=x.device)
    frames = torch.full((B * 4,), fill, dtype=torch.uint8, device=x.device)
    host = torch.as_tensor(lens, dtype=torch.int32)
    d = host.to(x.device)
    rc = lib.hificar_feat_forward(handle, x.data_ptr(), d.data_ptr(), host.data_ptr(), out.data_ptr(), frames.data_ptr(), B, L,
                                  ws.data_ptr() + off, n, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.hificar_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), frames.cpu().numpy()


@pytest.mark.parametrize("hop", O.MFCC_HOPS)
def test_mfcc_ragged_batch(mfcc_case, hop):
    wav, lens, ref = mfcc_case
    f = MFCC(sampling_rate=O.SR, hop_length=hop)
    feats, frames = f(dev(wav), lens)  # (NaN at and past every length)
    T = 1 + lens // hop
    assert feats.shape == (len(lens), 13, 1 + wav.shape[1] // hop) and feats.dtype == torch.float32
    assert frames.dtype == torch.int32 and frames.is_cuda and np.array_equal(frames.cpu().numpy(), T)
    again, _ = f(dev(wav), lens)
    assert torch.equal(feats, again)
    y = feats.cpu().numpy()
    assert np.isfinite(y).all()
    for b, n in enumerate(lens):
        c64 = ref[hop][b]
        assert c64.shape == (13, T[b]) and not y[b, :, T[b]:].any(), b
        c = y[b, :, :T[b]].astype(np.float64)
        rel = float(np.abs(c - c64).max() / np.abs(c64).max())
        zs = float(np.abs(O.zscore(c) - O.zscore(c64)).max())
        print(f"MFCC hop {hop} L {n}: rel {rel:.3g} (bar {O.BAR_MFCC_REL:g}), z-scored {zs:.3g} (bar {O.BAR_MFCC_Z:g})")
        assert rel < O.BAR_MFCC_REL and zs < O.BAR_MFCC_Z, (hop, n)
        alone, fr = f(dev(wav[b:b + 1, :n]))
        assert int(fr[0]) == T[b] and np.array_equal(alone[0].cpu().numpy(), y[b, :, :T[b]]), (hop, n)
    assert "libhificar.so" in open("/proc/self/maps").read()


def test_mfcc_reads_nothing_past_a_length_and_writes_every_element(mfcc_case):
    wav, lens, _ = mfcc_case
    clean = np.where(np.isnan(wav), np.float32(0.25), wav)
    for hop in O.MFCC_HOPS:
        f = MFCC(sampling_rate=O.SR, hop_length=hop)
        a, fa = run_native(f, wav, lens, 0xFF)
        b, fb = run_native(f, clean, lens, 0x00)
        assert np.array_equal(a, b) and np.array_equal(fa, fb), hop
        assert np.array_equal(fa.view(np.int32), 1 + lens // hop)


@pytest.mark.parametrize("case", O.LOGMEL_CASES, ids=lambda c: c[0])
def test_logmel(case):
    _, kw, lengths = case
    wav, lens = O.logmel_batch()
    assert tuple(lens) == lengths
    f = LogMel(O.SR, **kw)
    hop = f.hop_size
    feats, frames = f(dev(wav), lens)
    T = 1 + lens // hop
    assert feats.shape == (2, f.channels, 1 + wav.shape[1] // hop) and np.array_equal(frames.cpu().numpy(), T)
    assert torch.equal(feats, f(dev(wav), lens)[0])
    y = feats.cpu().numpy()
    for b, n in enumerate(lens):
        ref = O.logmel(wav[b, :n], O.SR, **kw)
        assert ref.shape == (f.channels, T[b]) and not y[b, :, T[b]:].any()
        err = float(np.abs(y[b, :, :T[b]].astype(np.float64) - ref).max())
        print(f"log-mel {case[0]} L {n}: {err:.3g} (bar {O.BAR_LOGMEL:g})")
        assert err < O.BAR_LOGMEL, (case[0], n)
        alone, _ = f(dev(wav[b, :n]))  # (L,): a batch of one
        assert alone.shape == (1, f.channels, T[b]) and np.array_equal(alone[0].cpu().numpy(), y[b, :, :T[b]])
    a, fa = run_native(f, wav, lens, 0xFF)
    b, fb = run_native(f, np.where(np.isnan(wav), np.float32(-3.0), wav), lens, 0x00)
    assert np.array_equal(a, b) and np.array_equal(fa, fb) and np.array_equal(a.view(np.float32).reshape(y.shape), y)


def test_speech_to_ema_end_to_end(mfcc_case, bigru13):
    """BiGRU.forward_lowrate(MFCC(wav), zscore=True) against the same model on the oracle's MFCCs (float64, rounded to float32)."""
    wav, lens, ref = mfcc_case
    model, _, params = bigru13
    for hop in O.MFCC_HOPS:
        f = MFCC(sampling_rate=O.SR, hop_length=hop)
        feats, frames = f(dev(wav), lens)
        T = 1 + lens // hop
        fed = np.zeros(tuple(feats.shape), dtype=np.float32)
        for b in range(len(lens)):
            fed[b, :, :T[b]] = ref[hop][b].astype(np.float32)
        with torch.no_grad():
            y = model.forward_lowrate(feats, lengths=frames, interp_factor=1, zscore=True).cpu().numpy()
            y_ref = model.forward_lowrate(dev(fed), lengths=T, interp_factor=1, zscore=True).cpu().numpy()
        assert y.shape == (len(lens), params["out_channels"], feats.shape[2])
        for b in range(len(lens)):
            err = rel_err(y[b, :, :T[b]], y_ref[b, :, :T[b]])
            print(f"speech -> EMA hop {hop} L {lens[b]}: {err:.3g} (bar {TOL_BIGRU:g})")
            assert err < TOL_BIGRU, (hop, b)
            assert not y[b, :, T[b]:].any()


def test_cli_from_wav_writes_the_same_bytes_at_any_batch_size(tmp_path, bigru13):
    model, sd, params = bigru13
    d = tmp_path / "mngu0_mfcc"
    d.mkdir()
    torch.save({"model": {"generator": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}}, d / "best_mel_ckpt.pkl")
    (d / "config.yml").write_text(yaml.safe_dump(dict(generator_type="BiGRU", generator_params=params, format="npy")))
    wavs = tmp_path / "wavs"
    wavs.mkdir()
    rng = np.random.default_rng(5)
    utts = {"uttA": 4000, "uttB": 801, "uttC": 2560, "uttD": 1234}
    pcm = {}
    for u, n in utts.items():
        pcm[u] = np.round(32767 * O.voiced(rng, n, 0.5)).astype("<i2")
        with wave.open(str(wavs / f"{u}.wav"), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(O.SR)
            w.writeframes(pcm[u].tobytes())
    for bs in (1, 3):
        PE.main([str(d), str(wavs), str(tmp_path / f"out{bs}"), "--from-wav", "--batch-size", str(bs), "--verbose", "0"])
    f = MFCC(sampling_rate=O.SR, hop_length=80)
    for u, n in utts.items():
        a, b = (tmp_path / "out1" / f"{u}.npy").read_bytes(), (tmp_path / "out3" / f"{u}.npy").read_bytes()
        assert a == b, u
        y = np.load(tmp_path / "out1" / f"{u}.npy")
        assert y.shape == (1 + n // 80, 12) and y.dtype == np.float32
        feats, frames = f(dev(pcm[u].astype(np.float32) / np.float32(32768.0)))
        with torch.no_grad():
            direct = model.forward_lowrate(feats, lengths=frames, interp_factor=1, zscore=True)[0].t().cpu().numpy()
        assert np.array_equal(y, direct), u
