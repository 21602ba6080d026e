"""Speech features (``articulatory_amd.features``, ``hificar_feat_*``, ``predict_ema --from-wav``) without a GPU: the float64 restatement
against an independent route, the float32 emulation that sets the GPU tests' bars, the refusals and signatures of the two classes, the C
entry points' argument checks, the wav reader and the CLI's plans.

The bars (tests/speech_features_oracle.py restated in float32 over exactly the inputs of tests/test_gpu_speech_features.py; each bar is
four times the emulation's worst error, rounded up to one significant digit — the emulation sits at a quarter of its bar, as the bf16
arithmetics' bars were placed, because numpy's summation order is not the MFMA tiles'):

    quantity                                   float32 emulation    bar
    MFCC, relative to the utterance's max|c|   1.28e-7              6e-7
    MFCC, z-scored (absolute)                  4.80e-7              2e-6
    log-mel (absolute, in the log's own base)  8.36e-6              4e-5

No element is excluded from any comparison: the floor at amin and the clamp at max - top_db are continuous.
"""

import copy
import ctypes
import inspect
import json
import os
import pickle
import wave

import numpy as np
import pytest
import torch
import yaml

import speech_features_oracle as O
from articulatory_amd import _native
from articulatory_amd.bin import predict_ema as PE
from articulatory_amd.features import MFCC, LogMel
from articulatory_amd.utils.mel import mel_filterbank
from conftest import REPO

from speech_features_oracle import BAR_LOGMEL, BAR_MFCC_REL, BAR_MFCC_Z  # 6e-7, 2e-6, 4e-5: the table above


# ---------------------------------------------------------------------------------------------- the restatement
def _torch_power(y, n_fft, hop, win_length):
    w = torch.hann_window(win_length, periodic=True, dtype=torch.float64)
    S = torch.stft(torch.from_numpy(np.asarray(y, dtype=np.float64)), n_fft, hop_length=hop, win_length=win_length, window=w, center=True,
                   pad_mode="reflect", return_complex=True)
    return (S.real ** 2 + S.imag ** 2).numpy()  # (nf, T)


def test_oracle_agrees_with_an_independent_route():
    """torch.stft in float64 -> the basis of utils/mel.py -> scipy.fftpack.dct: <= 1e-10 (probed: 1.7e-13)."""
    from scipy.fftpack import dct

    wav, lens = O.mfcc_batch()
    worst = 0.0
    for hop in O.MFCC_HOPS:
        for b in (0, 3, 5):
            y = wav[b, :lens[b]]
            mel = mel_filterbank(O.SR, 320, 40, 0.0, O.SR / 2).astype(np.float64) @ _torch_power(y, 320, hop, 320)
            db = 10.0 * np.log10(np.maximum(1e-10, mel))
            db = np.maximum(db, db.max() - 80.0)
            ref = dct(db, axis=0, type=2, norm="ortho")[:13]
            got = O.mfcc(y, O.SR, hop_length=hop)
            assert got.shape == ref.shape == (13, 1 + lens[b] // hop)
            worst = max(worst, float(np.abs(got - ref).max()))
    wav, lens = O.logmel_batch()
    for _, kw, _ in O.LOGMEL_CASES:
        n_fft, hop, win = kw.get("fft_size", 1024), kw.get("hop_size", 256), kw.get("win_length") or kw.get("fft_size", 1024)
        fb = mel_filterbank(O.SR, n_fft, kw.get("num_mels", 80), kw.get("fmin", 0), O.SR / 2).astype(np.float64)
        log = {None: np.log, 2.0: np.log2, 10.0: np.log10}[kw.get("log_base", 10.0)]
        ref = log(np.maximum(1e-10, fb @ np.sqrt(_torch_power(wav[0, :lens[0]], n_fft, hop, win))))
        worst = max(worst, float(np.abs(O.logmel(wav[0, :lens[0]], O.SR, **kw) - ref).max()))
    print(f"oracle against the independent route: {worst:.3g}")
    assert worst <= 1e-10


def test_the_test_batch_reaches_the_floor_and_the_clamp():
    wav, lens = O.mfcc_batch()
    assert tuple(lens) == O.MFCC_LENGTHS and all(np.isnan(wav[b, n:]).all() and np.isfinite(wav[b, :n]).all() for b, n in enumerate(lens))
    assert abs(np.abs(wav[4, :lens[4]]).max() - 1.0) < 1e-6 and np.abs(wav[3, :lens[3]]).max() < 1e-3
    db = O.mfcc_db(wav[5, :lens[5]], O.SR, hop_length=80)
    assert (db == db.max() - 80.0).any() and db.max() - 80.0 > -100.0  # silent frames: floored at amin (-100 dB), then clamped
    assert 1 + 161 // 80 == 3 and 1 + 2560 // 80 == 33 and 1 + 2640 // 80 == 34 and 1 + 800 // 160 != 1 + 799 // 160


def test_float32_emulation_sets_the_bars():
    rel, zs, lm = O.emulation_errors()
    print(f"float32 emulation: MFCC rel {rel:.3g}, z-scored {zs:.3g}, log-mel {lm:.3g}")
    # the module's figures are this computation's on the machine the bars were set on; another BLAS sums in another order, which may move
    # the emulation by a fraction: it stays at about a quarter of its bar
    for worst, bar in ((rel, BAR_MFCC_REL), (zs, BAR_MFCC_Z), (lm, BAR_LOGMEL)):
        assert 4.0 * worst <= 1.25 * bar and bar <= 10.0 * worst, (worst, bar)
    assert O.one_digit_up(4 * 1.28e-7) == BAR_MFCC_REL and O.one_digit_up(4 * 4.80e-7) == BAR_MFCC_Z and O.one_digit_up(4 * 8.36e-6) == BAR_LOGMEL


# ---------------------------------------------------------------------------------------------- the classes
def test_signatures_and_refusals():
    sig = inspect.signature(MFCC.__init__).parameters
    assert [(k, sig[k].default) for k in list(sig)[1:6]] == [("sampling_rate", 16000), ("n_mfcc", 13), ("n_mels", 40), ("n_fft", 320),
                                                             ("hop_length", 160)]
    sig = inspect.signature(LogMel.__init__).parameters
    assert [(k, sig[k].default) for k in list(sig)[2:11]] == [("fft_size", 1024), ("hop_size", 256), ("win_length", None), ("window", "hann"),
                                                              ("num_mels", 80), ("fmin", None), ("fmax", None), ("eps", 1e-10), ("log_base", 10.0)]
    assert list(sig)[1] == "sampling_rate" and sig["sampling_rate"].default is inspect.Parameter.empty
    m, l = MFCC(), LogMel(16000)
    assert isinstance(m, torch.nn.Module) and not list(m.parameters()) and not list(l.parameters()) and not m.state_dict()
    assert (m.channels, l.channels, m.frames(161), l.frames(8192)) == (13, 80, 2, 33)
    assert np.array_equal(m.melmat, mel_filterbank(16000, 320, 40, 0.0, 8000.0)) and np.array_equal(l.melmat, mel_filterbank(16000, 1024, 80, 0, 8000.0))
    with pytest.raises(NotImplementedError, match="window"):
        LogMel(16000, window="hamming")
    with pytest.raises(ValueError, match="is not supported"):
        LogMel(16000, log_base=3.0)
    with pytest.raises(ValueError, match="multiple of 32"):
        MFCC(n_fft=400)
    with pytest.raises(ValueError, match="n_mfcc"):
        MFCC(n_mfcc=41)
    with pytest.raises(ValueError, match="mel bands"):
        LogMel(16000, num_mels=129)
    for f in (m, l):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(torch.zeros(2, 4000))
    # the refusals behind the device check, on a stand-in that says it is on the device
    class OnDevice(torch.Tensor):
        device = torch.device("cuda", 0)

    def fake(shape, grad=False):
        t = torch.zeros(shape).as_subclass(OnDevice)
        t.requires_grad_(grad)
        return t

    with pytest.raises(RuntimeError, match="requires grad"):
        m(fake((2, 4000), grad=True))
    with pytest.raises(ValueError, match="more than n_fft / 2 = 160"):
        m(fake((2, 160)))
    with pytest.raises(ValueError, match="a length of 160"):
        m(fake((2, 4000)), lengths=[4000, 160])
    with pytest.raises(RuntimeError, match="3 entries for a batch of 2"):
        m(fake((2, 4000)), lengths=[4000, 300, 300])
    with pytest.raises(RuntimeError, match=r"lengths must lie in \[1, 4000\]"):
        m(fake((2, 4000)), lengths=[4001, 300])
    with pytest.raises(RuntimeError, match=r"\(B, L\) or \(L,\)"):
        m(fake((2, 1, 4000)))


def test_copies_and_pickles_never_share_a_handle():
    m = MFCC(hop_length=80)
    h = m._native_handle(torch.device("cuda", 0))  # (creation touches no device)
    assert h is not None and m._native_handle(torch.device("cuda", 0)) is h
    c, p = copy.deepcopy(m), pickle.loads(pickle.dumps(m))
    for other in (c, p):
        assert other._handle is None and other._workspace_buf is None and other._cfg.hop_size == 80 and np.array_equal(other.melmat, m.melmat)
        assert other._native_handle(torch.device("cuda", 0)).value != h.value
    m._invalidate()
    assert m._handle is None


# ---------------------------------------------------------------------------------------------- the C ABI
def test_c_entry_points_refuse_bad_arguments():
    lib = _native.load_library()
    hdr = open(os.path.join(REPO, "include", "hificar.h")).read()
    for s in ("hificar_feat_create", "hificar_feat_destroy", "hificar_feat_engine", "hificar_feat_frames", "hificar_feat_workspace_bytes", "hificar_feat_forward"):
        assert s in _native.SYMBOLS and s in hdr
    assert f"#define HIFICAR_FEAT_MAX_MELS {_native.FEAT_MAX_MELS}" in hdr and f"#define HIFICAR_FEAT_MFCC {_native.FEAT_MFCC}" in hdr
    fb = mel_filterbank(16000, 320, 40, 0.0, 8000.0)
    fbp = fb.ctypes.data_as(ctypes.c_void_p)

    def create(**kw):
        v = dict(kind=_native.FEAT_MFCC, fft_size=320, hop_size=80, win_length=320, num_mels=40, n_mfcc=13, amin=1e-10, top_db=80.0, log_base=10)
        v.update(kw)
        h = ctypes.c_void_p()
        rc = lib.hificar_feat_create(ctypes.byref(_native.HificarFeatConfig(*v.values())), fbp, ctypes.byref(h))
        return rc, h

    for kw, msg in ((dict(kind=2), b"kind"), (dict(fft_size=400), b"multiple of 32"), (dict(hop_size=0), b"hop_size"), (dict(win_length=321), b"win_length"),
                    (dict(num_mels=129), b"num_mels"), (dict(n_mfcc=41), b"n_mfcc"), (dict(n_mfcc=0), b"n_mfcc"), (dict(amin=0.0), b"amin"),
                    (dict(kind=_native.FEAT_LOGMEL, log_base=3), b"log_base")):
        rc, _ = create(**kw)
        assert rc == -1 and msg in lib.hificar_last_error(), kw
    assert lib.hificar_feat_create(None, fbp, ctypes.byref(ctypes.c_void_p())) == -1 and b"null" in lib.hificar_last_error()
    rc, h = create()
    assert rc == 0
    try:
        assert [lib.hificar_feat_frames(h, n) for n in (160, 161, 799, 800, 2560)] == [0, 3, 10, 11, 33]
        assert lib.hificar_feat_workspace_bytes(h, 0, 4000) == 0 and lib.hificar_feat_workspace_bytes(h, 2, 160) == 0
        assert lib.hificar_feat_workspace_bytes(h, 65535, 1 << 20) == 0
        # A [rows][320] + S [rows][2 * 192] + V [M][40] + one maximum per utterance, rows = M rounded up to 256, each buffer to 1 KiB
        M, rows = 6 * 51, 512
        assert lib.hificar_feat_workspace_bytes(h, 6, 4000) == rows * 320 * 4 + rows * 384 * 4 + -(-M * 40 * 4 // 1024) * 1024 + 1024
        fn, fake = lib.hificar_feat_forward, 1 << 20
        big = 1 << 40
        assert fn(None, fake, None, None, fake, None, 2, 4000, fake, big, None) == -1 and b"null" in lib.hificar_last_error()
        assert fn(h, None, None, None, fake, None, 2, 4000, fake, big, None) == -1 and b"null" in lib.hificar_last_error()
        assert fn(h, fake, None, None, fake, None, 2, 160, fake, big, None) == -1 and b"reflect padding" in lib.hificar_last_error()
        assert fn(h, fake, None, None, fake, None, 0, 4000, fake, big, None) == -1 and b"out of range" in lib.hificar_last_error()
        assert fn(h, fake, None, None, fake, None, 65535, 1 << 20, fake, big, None) == -1 and b"out of range" in lib.hificar_last_error()
        lens = np.asarray([4000, 160], dtype=np.int32)
        assert fn(h, fake, None, lens.ctypes.data, fake, None, 2, 4000, fake, big, None) == -1 and b"lengths_host" in lib.hificar_last_error()
        assert fn(h, fake, fake, lens.ctypes.data, fake, None, 2, 4000, fake, big, None) == -1 and b"lengths[1]=160" in lib.hificar_last_error()
        lens[1] = 4001
        assert fn(h, fake, fake, lens.ctypes.data, fake, None, 2, 4000, fake, big, None) == -1 and b"lengths[1]=4001" in lib.hificar_last_error()
        assert fn(h, fake, None, None, fake, None, 2, 4000, fake + 8, big, None) == -1 and b"aligned" in lib.hificar_last_error()
        assert fn(h, fake, None, None, fake, None, 2, 4000, None, big, None) == -1 and b"aligned" in lib.hificar_last_error()
        need = lib.hificar_feat_workspace_bytes(h, 2, 4000)
        assert fn(h, fake, None, None, fake, None, 2, 4000, fake, need - 1, None) == -4 and b"too small" in lib.hificar_last_error()
    finally:
        lib.hificar_feat_destroy(h)
    lib.hificar_feat_destroy(None)


# ---------------------------------------------------------------------------------------------- the wav reader and the CLI
def write_wav(path, samples, sr=16000, channels=1, width=2):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(sr)
        w.writeframes(np.asarray(samples).tobytes())


def test_wav_reader(tmp_path):
    pcm = np.asarray([0, 1, -1, 32767, -32768, 12345, -2], dtype="<i2")
    write_wav(tmp_path / "a.wav", pcm, sr=22050)
    y, sr = PE.read_wav(str(tmp_path / "a.wav"))
    assert sr == 22050 and y.dtype == np.float32 and np.array_equal(y.astype(np.float64), pcm.astype(np.float64) / 32768.0)
    assert PE.wav_info(str(tmp_path / "a.wav")) == (22050, 7)
    write_wav(tmp_path / "stereo.wav", np.zeros(8, dtype="<i2"), channels=2)
    write_wav(tmp_path / "eight.wav", np.zeros(8, dtype=np.uint8), width=1)
    data = open(tmp_path / "a.wav", "rb").read()
    (tmp_path / "cut.wav").write_bytes(data[:-5])
    (tmp_path / "junk.wav").write_bytes(b"not a wav file at all")
    for name, msg in (("stereo.wav", "2 channel"), ("eight.wav", "8 bit"), ("cut.wav", "truncated"), ("junk.wav", "not a PCM wav")):
        with pytest.raises(ValueError, match=msg) as e:
            PE.read_wav(str(tmp_path / name))
        assert name in str(e.value)
    assert PE.list_wavs(str(tmp_path))[0] == ("a", str(tmp_path / "a.wav"))
    scp = tmp_path / "wav.scp"
    scp.write_text(f"one {tmp_path / 'a.wav'}\n\ntwo {tmp_path / 'cut.wav'}\n")
    assert PE.list_wavs(str(scp)) == [("one", str(tmp_path / "a.wav")), ("two", str(tmp_path / "cut.wav"))]


def test_cli_plans_from_wav(tmp_path, capsys):
    assert PE.derive_hop_length("exp/hprc_f1_mfcc") == 160 and PE.derive_hop_length("exp/mngu0_mfcc/") == 80
    params = dict(in_channels=13, hidden_size=64, out_channels=12, use_tanh=True)
    wavs = tmp_path / "wavs"
    wavs.mkdir()
    write_wav(wavs / "uttB.wav", np.zeros(1600, dtype="<i2"))
    write_wav(wavs / "uttA.wav", np.zeros(801, dtype="<i2"), sr=8000)

    def plan(name, *flags):
        d = tmp_path / name
        if not d.exists():
            d.mkdir()
            (d / "config.yml").write_text(yaml.safe_dump(dict(generator_type="BiGRU", generator_params=params, format="npy")))
        PE.main([str(d), str(wavs), str(tmp_path / "never"), "--dry-run", "--verbose", "0", *flags])
        lines = capsys.readouterr().out.strip().splitlines()
        assert len(lines) == 1
        return json.loads(lines[0])

    p = plan("mngu0_mfcc", "--from-wav")
    assert (p["front_end"], p["hop_length"], p["rates"], p["utterances"]) == ("mfcc", 80, [8000, 16000], ["uttA", "uttB"])
    assert (p["interp_factor"], p["zscore"], p["batch_size"], p["precision"]) == (1, True, 1, "f32")
    assert (p["n_mfcc"], p["n_mels"], p["n_fft"], p["samples"], p["frames"]) == (13, 40, 320, 2401, 11 + 21)
    p = plan("hprc_f1_mfcc", "--from-wav", "--no-zscore", "--batch-size", "3")
    assert (p["hop_length"], p["zscore"], p["batch_size"], p["frames"]) == (160, False, 3, 6 + 11)
    assert plan("hprc_f1_mfcc", "--from-wav", "--hop-length", "40")["hop_length"] == 40
    with pytest.raises(NotImplementedError, match="SSL extraction is not built"):
        plan("mngu0_h2", "--from-wav")
    with pytest.raises(ValueError, match="--hop-length belongs to --from-wav"):
        plan("mngu0_mfcc", "--hop-length", "80")
    write_wav(wavs / "uttC.wav", np.zeros(16, dtype="<i2"), channels=2)
    with pytest.raises(ValueError, match="uttC.wav"):
        plan("mngu0_mfcc", "--from-wav")
    assert not (tmp_path / "never").exists()
