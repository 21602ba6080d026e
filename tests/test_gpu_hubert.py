"""``features.HuBERT`` (the HuBERT encoder of the large family) on a MI355X, through the C ABI, against the float64 restatement
tests/hubert_oracle.py, which tests/test_hubert_host.py pins to the ``transformers`` library's ``HubertModel``.  ``pytest -m gpu``.
Values: 2e-5 of max|y| per tensor, the project's exact-fp32 bar.
"""

import json
import wave

import numpy as np
import pytest
import torch
import yaml

import hubert_oracle as O
from conftest import rel_err
from articulatory_amd import _native
from articulatory_amd.bin import predict_ema as PE
from articulatory_amd.features import HuBERT
from articulatory_amd.utils.synth import synth_bigru_state_dict, synth_hubert_state_dict
from test_hubert_host import LARGE, SEED, TINY

pytestmark = pytest.mark.gpu
TOL = 2e-5
DEV = "cuda:0"
TAPS = {"extractor.0": "conv", "extract_features": "conv", "feature_projection": "hidden", "pos_conv": "hidden"}


def samples(frames):
    return 400 + 320 * (frames - 1)


_MODELS = {}


def model_of(tag, config, **kw):
    """(device model, numpy state_dict) of a configuration, built once per module."""
    if tag not in _MODELS:
        assert torch.cuda.is_available()
        sd = synth_hubert_state_dict(config, seed=SEED)
        m = HuBERT(config, **kw)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        _MODELS[tag] = (m.to(DEV), sd)
    return _MODELS[tag]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def check(tag, got, ref):
    err = rel_err(got, ref)
    print(f"{tag}: rel_err {err:.3e}")
    assert got.shape == ref.shape and err < TOL, (tag, err)


# 1 .. 149 frames: the attention's query-tile and key-block edges (63, 64, 65; 128, 129), the positional conv on a sequence shorter than its
# padding (1, 63), equal to its kernel (128) and one past it (129), two row tiles of it (129, 149); 719 / 720 samples: where the frame count steps
@pytest.mark.parametrize("L", [samples(n) for n in (1, 63, 64, 65, 128, 129, 149)] + [719, 720])
def test_tiny_every_output_and_tap(L):
    m, sd = model_of("tiny", TINY)
    wav = O.synth_wav(SEED + L, L)
    ref = O.forward(sd, TINY, wav)
    T, T0, C, H = O.frames(L), (L - 10) // 5 + 1, 64, 128
    bufs = {k: torch.full((1, T0 if k == "extractor.0" else T, C if w == "conv" else H), float("nan"), device=DEV) for k, w in TAPS.items()}
    bufs["layers.0"] = torch.full((1, T, H), float("nan"), device=DEV)
    for k, v in bufs.items():
        m.debug_tap(k, v)
    try:
        out, frames = m(dev(wav)[None])
    finally:
        m.debug_tap(None, None)
    assert out.shape == (1, H, T) and frames.tolist() == [T] and frames.dtype == torch.int32
    check("last_hidden_state", out[0].cpu().numpy().T, ref["last_hidden_state"])
    for k in TAPS:
        check(k, bufs[k][0].cpu().numpy(), ref[k])
    check("layers.0", bufs["layers.0"][0].cpu().numpy(), ref["hidden_states"][1])
    for k in (0, 1):
        check(f"hidden_states[{k}]", m(dev(wav), layer=k)[0][0].cpu().numpy().T, ref["hidden_states"][k])


def ragged_batch():
    lens = [samples(n) for n in (129, 65, 1, 12)]
    wavs = [O.synth_wav(SEED + 7 * i, l) for i, l in enumerate(lens)]
    padded = np.zeros((len(lens), max(lens)), dtype=np.float32)
    for i, w in enumerate(wavs):
        padded[i, :len(w)] = w
    return lens, wavs, padded


def test_ragged_batch_is_bitwise_each_utterance_alone_also_on_dirty_scratch():
    m, sd = model_of("tiny", TINY)
    lens, wavs, padded = ragged_batch()
    out, frames = m(dev(padded), lengths=lens)
    assert frames.tolist() == [129, 65, 1, 12] and out.shape == (4, 128, 129)
    m._workspace_buf.fill_(255)  # every float of the scratch a NaN
    again, _ = m(dev(padded), lengths=torch.tensor(lens))
    assert torch.equal(out, again)
    for i, (w, n) in enumerate(zip(wavs, frames.tolist())):
        alone, _ = m(dev(w)[None])
        assert torch.equal(out[i, :, :n], alone[0]), i
        assert not out[i, :, n:].any(), i
        check(f"utterance {i}", out[i, :, :n].cpu().numpy().T, O.forward(sd, TINY, w)["last_hidden_state"])
    for k in (0, 1):
        hk, _ = m(dev(padded), lengths=lens, layer=k)
        for i, (w, n) in enumerate(zip(wavs, frames.tolist())):
            assert torch.equal(hk[i, :, :n], m(dev(w), layer=k)[0][0]) and not hk[i, :, n:].any()
    # the extractor over sub-batches of 3 + 1 and of 1 utterance: the same bytes (the default budget holds all four in one)
    for n in (3, 1, 0):
        m._call("_debug_sub_batch", m._native_handle(), n)
        sub, _ = m(dev(padded), lengths=lens)
        assert torch.equal(out, sub), n
    with pytest.raises(ValueError, match="under 400 samples"):
        m(dev(padded), lengths=[399] + lens[1:])
    with pytest.raises(RuntimeError, match="lengths must lie"):
        m(dev(padded), lengths=[padded.shape[1] + 1] + lens[1:])


def profiled(m, fn):
    eng = m.engine()
    lib = m._lib
    _native.check(lib.hificar_profile_begin(eng), "hificar_profile_begin")
    out = fn()
    rows, n = _native.profile_rows(lib, eng, 512)
    assert n < 512
    return out, {r["name"]: r["launches"] for r in rows}


@pytest.mark.parametrize("layer", [0, 1, -1])
def test_layers_above_the_requested_one_are_not_launched(layer):
    m, sd = model_of("tiny", TINY)
    L = samples(65)
    wav = O.synth_wav(SEED + L, L)
    (out, _), rows = profiled(m, lambda: m(dev(wav), layer=layer))
    ref = O.forward(sd, TINY, wav)["hidden_states"][layer]
    check(f"layer={layer}", out[0].cpu().numpy().T, ref)
    ran = 2 if layer < 0 else layer
    assert rows.get("hubert_attn_kernel", 0) == ran and rows.get("hubert_gelu_kernel", 0) == ran
    assert rows["hubert_posconv_kernel"] == 1 and rows["hubert_conv0_kernel"] == 1
    # LayerNorms without GELU: the projection's, two per layer run, the encoder's own for layer = -1 alone
    assert rows["hubert_ln_kernel"] == 1 + 2 * ran + (1 if layer < 0 else 0) and rows["hubert_ln_kernel<gelu>"] == 6


def test_large_widths_four_layers():
    """conv 512 / hidden 1024 / 16 heads / FFN 4096: the real tile shapes, 64 channels per positional group; 1 s (49 frames), 4 layers."""
    config = dict(LARGE, num_hidden_layers=4)
    m, sd = model_of("wide", config)
    wav = O.synth_wav(SEED + 1, 16000)
    ref = O.forward(sd, config, wav)
    out, frames = m(dev(wav))
    assert frames.tolist() == [49]
    check("wide last_hidden_state", out[0].cpu().numpy().T, ref["last_hidden_state"])
    check("wide hidden_states[2]", m(dev(wav), layer=2)[0][0].cpu().numpy().T, ref["hidden_states"][2])


def test_tiny_width_24_layers():
    config = dict(TINY, num_hidden_layers=24)
    m, sd = model_of("deep", config)
    wav = O.synth_wav(SEED + 2, 48000)
    out, _ = m(dev(wav))
    check("deep last_hidden_state", out[0].cpu().numpy().T, O.forward(sd, config, wav)["last_hidden_state"])


def test_conv_bias_false():
    config = dict(TINY, conv_bias=False, mask_time_prob=0.0)
    m, sd = model_of("nobias", config)
    assert "masked_spec_embed" not in sd and "feature_extractor.conv_layers.3.conv.bias" not in sd
    wav = O.synth_wav(SEED + 3, samples(20))
    check("conv_bias=False", m(dev(wav))[0][0].cpu().numpy().T, O.forward(sd, config, wav)["last_hidden_state"])


@pytest.mark.parametrize("normalize", [True, False])
def test_normalisation_with_an_offset_and_a_small_amplitude(normalize):
    """Amplitude 3e-4 on an offset of 0.3: the variance is of the order of norm_eps = 1e-7, so the eps shows; off: the samples as they are."""
    m, sd = model_of(f"norm{normalize}", TINY, normalize=normalize)
    wav = O.synth_wav(SEED + 4, samples(30), amplitude=3e-4, offset=0.3)
    assert float(np.var(wav.astype(np.float64))) < 1e-6
    ref = O.forward(sd, TINY, wav, do_normalize=normalize)
    out, _ = m(dev(wav))
    check(f"normalize={normalize}", out[0].cpu().numpy().T, ref["last_hidden_state"])
    # what the case must tell apart: on, the same without the eps; off, the normalised run
    other = O.forward(sd, TINY, wav, do_normalize=True, norm_eps=0.0 if normalize else O.NORM_EPS)["last_hidden_state"]
    assert rel_err(other, ref["last_hidden_state"]) > 10 * TOL  # (the case tells the two apart)


def write_wav(path, y):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.clip(np.round(y * 32768.0), -32768, 32767).astype("<i2").tobytes())


def test_predict_ema_end_to_end(tmp_path):
    """predict_ema.main on a temporary foo_h2 directory (a BiGRU of in_channels 128), a tiny HuBERT directory and four wavs of unequal
    length: the files equal HuBERT -> forward_lowrate(interp_factor=4) composed by hand, and --batch-size 1 and 3 write identical bytes."""
    from articulatory_amd.models import BiGRU

    params = dict(in_channels=128, hidden_size=64, out_channels=12, use_tanh=False)
    d = tmp_path / "foo_h2"
    d.mkdir()
    bsd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth_bigru_state_dict(params, seed=5).items()}
    torch.save({"model": {"generator": bsd}}, d / PE.CHECKPOINT)
    (d / "config.yml").write_text(yaml.safe_dump(dict(generator_type="BiGRU", generator_params=params, format="npy")))
    hub = tmp_path / "hubert"
    hub.mkdir()
    (hub / "config.json").write_text(json.dumps(dict(TINY, model_type="hubert")))
    torch.save({k: torch.from_numpy(v) for k, v in synth_hubert_state_dict(TINY, seed=SEED).items()}, hub / "pytorch_model.bin")
    wavs = tmp_path / "wavs"
    wavs.mkdir()
    lens = {"uttA": 24000, "uttB": 8117, "uttC": 400, "uttD": 4001}
    for i, (u, l) in enumerate(lens.items()):
        write_wav(wavs / f"{u}.wav", O.synth_wav(SEED + 11 * i, l, amplitude=0.3))
    for bs in (1, 3):
        PE.main([str(d), str(wavs), str(tmp_path / f"out{bs}"), "--from-wav", "--ssl-model", str(hub), "--batch-size", str(bs), "--verbose", "0"])
    hubert = HuBERT.from_pretrained(str(hub)).to(DEV)
    model = BiGRU(**params)
    model.load_state_dict(bsd)
    model = model.eval().to(DEV)
    for u, l in lens.items():
        y, sr = PE.read_wav(str(wavs / f"{u}.wav"))
        assert sr == 16000 and len(y) == l
        feats, frames = hubert(dev(y)[None])
        want = model.forward_lowrate(feats, lengths=frames, interp_factor=4)[0].T.cpu().numpy()
        a, b = np.load(tmp_path / "out1" / f"{u}.npy"), np.load(tmp_path / "out3" / f"{u}.npy")
        assert a.shape == (4 * O.frames(l), 12) and a.dtype == np.float32
        assert np.array_equal(a, want), u
        assert (tmp_path / "out1" / f"{u}.npy").read_bytes() == (tmp_path / "out3" / f"{u}.npy").read_bytes(), u
