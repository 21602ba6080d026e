"""``features.HuBERT(precision="bf16x3" | "bf16x3a")`` on a MI355X, through the C ABI, against the float64 restatement tests/hubert_oracle.py.
``pytest -m gpu``.  Values: 2e-4 of max|y| per tensor, the project's bf16x3 bar — tests/test_hubert_bf16x3_host.py shows on the CPU that the
arithmetic itself stays under 1e-4 on these inputs (1.4e-5 .. 3.1e-5), so the bar is not fitted to a device result.
"""

import json

import numpy as np
import pytest
import torch
import yaml

import hubert_oracle as O
from conftest import rel_err
from articulatory_amd.bin import predict_ema as PE
from articulatory_amd.features import HuBERT
from articulatory_amd.utils.synth import synth_bigru_state_dict, synth_hubert_state_dict
from test_gpu_hubert import DEV, dev, profiled, ragged_batch, samples, write_wav
from test_hubert_host import LARGE, SEED, TINY

pytestmark = pytest.mark.gpu
TOL = 2e-4
BOTH = ("bf16x3", "bf16x3a")
TAPS = {"extract_features": "conv", "feature_projection": "hidden", "pos_conv": "hidden"}

_MODELS, _REFS = {}, {}


def model_of(tag, config, precision, gain=1.0):
    """(device model, numpy state_dict) of a configuration and arithmetic, built once per module."""
    key = (tag, precision)
    if key not in _MODELS:
        assert torch.cuda.is_available()
        sd = synth_hubert_state_dict(config, seed=SEED, gain=gain)
        m = HuBERT(config, precision=precision)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        assert m.precision == precision
        _MODELS[key] = (m.to(DEV), sd)
    return _MODELS[key]


def reference(tag, sd, config, wav):
    """The float64 forward of a case, computed once and shared by the two arithmetics."""
    if tag not in _REFS:
        _REFS[tag] = O.forward(sd, config, wav)
    return _REFS[tag]


def check(tag, got, ref):
    err = rel_err(got, ref)
    print(f"{tag}: rel_err {err:.3e}")
    assert got.shape == ref.shape and err < TOL, (tag, err)


# the frame counts of tests/test_gpu_hubert.py: the attention's query-tile and key-block edges (63, 64, 65; 128, 129), a one-row window
# layer (1 frame: layer 6 reads one window), the extractor in split rows throughout; 719 / 720 samples: where the frame count steps
@pytest.mark.parametrize("L", [samples(n) for n in (1, 63, 64, 65, 128, 129, 149)] + [719, 720])
@pytest.mark.parametrize("precision", BOTH)
def test_tiny_every_output_and_tap(precision, L):
    m, sd = model_of("tiny", TINY, precision)
    wav = O.synth_wav(SEED + L, L)
    ref = reference(("tiny", L), sd, TINY, wav)
    T, C, H = O.frames(L), 64, 128
    bufs = {k: torch.full((1, T, C if w == "conv" else H), float("nan"), device=DEV) for k, w in TAPS.items()}
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


@pytest.mark.parametrize("precision", BOTH)
def test_ragged_batch_is_bitwise_each_utterance_alone_also_on_dirty_scratch(precision):
    m, sd = model_of("tiny", TINY, precision)
    lens, wavs, padded = ragged_batch()
    out, frames = m(dev(padded), lengths=lens)
    assert frames.tolist() == [129, 65, 1, 12] and out.shape == (4, 128, 129)
    m._workspace_buf.fill_(255)  # every float of the scratch a NaN, every bf16 too
    again, _ = m(dev(padded), lengths=torch.tensor(lens))
    assert torch.equal(out, again)
    for i, (w, n) in enumerate(zip(wavs, frames.tolist())):
        alone, _ = m(dev(w)[None])
        assert torch.equal(out[i, :, :n], alone[0]), i
        assert not out[i, :, n:].any(), i
        check(f"utterance {i}", out[i, :, :n].cpu().numpy().T, reference(("ragged", i), sd, TINY, w)["last_hidden_state"])
    for n in (3, 1, 0):  # the extractor over sub-batches of 3 + 1 and of 1 utterance: the same bytes
        m._call("_debug_sub_batch", m._native_handle(), n)
        sub, _ = m(dev(padded), lengths=lens)
        assert torch.equal(out, sub), n


def _conv_rows(rows, family):
    return sum(v for k, v in rows.items() if k.startswith(family))


@pytest.mark.parametrize("layer", [0, 1, -1])
def test_which_kernels_an_arithmetic_launches(layer):
    L = samples(65)
    wav = O.synth_wav(SEED + L, L)
    ran = 2 if layer < 0 else layer
    gemms = 6 + 1 + 4 * ran
    # f32: none of the new kernels or instantiations
    m, _ = model_of("tiny", TINY, "f32")
    _, rows = profiled(m, lambda: m(dev(wav), layer=layer))
    assert not [k for k in rows if "split" in k or "attn16" in k or "bf16x3" in k], rows
    assert rows.get("hubert_attn_kernel", 0) == ran and rows.get("hubert_gelu_kernel", 0) == ran and rows["hubert_conv0_kernel"] == 1
    assert _conv_rows(rows, "conv_f32") == gemms
    for precision in BOTH:
        m, sd = model_of("tiny", TINY, precision)
        (out, _), rows = profiled(m, lambda: m(dev(wav), layer=layer))
        check(f"{precision} layer={layer}", out[0].cpu().numpy().T, reference(("tiny", L), sd, TINY, wav)["hidden_states"][layer])
        assert _conv_rows(rows, "conv_bf16x3") == gemms and _conv_rows(rows, "conv_f32") == 0 and _conv_rows(rows, "conv_sk") == 0, rows
        assert "hubert_attn_kernel" not in rows and "hubert_gelu_kernel" not in rows and "hubert_conv0_kernel" not in rows
        if precision == "bf16x3":
            assert rows.get("hubert_attn_kernel<split>", 0) == ran and "hubert_attn16_kernel" not in rows
        else:
            assert rows.get("hubert_attn16_kernel", 0) == ran and "hubert_attn_kernel<split>" not in rows
        assert rows.get("hubert_gelu_split_kernel", 0) == ran and rows["hubert_conv0_kernel<split>"] == 1 and rows["hubert_posconv_kernel"] == 1
        # split LayerNorms: the projection's and two per layer run; fp32: the encoder's own for layer = -1 alone; extractor: five split, layer 6's fp32
        assert rows["hubert_ln_kernel<split>"] == 1 + 2 * ran and rows.get("hubert_ln_kernel", 0) == (1 if layer < 0 else 0)
        assert rows["hubert_ln_kernel<gelu,split>"] == 5 and rows["hubert_ln_kernel<gelu>"] == 1


def test_set_precision_and_back_gives_the_same_bytes():
    m, sd = model_of("switch", TINY, "f32")
    L = samples(65)
    wav = dev(O.synth_wav(SEED + L, L))
    before, _ = m(wav)
    ws = m.workspace_bytes(1, L)
    m.set_precision("bf16x3")
    mid, _ = m(wav)
    assert m.precision == "bf16x3" and not torch.equal(before, mid) and m.workspace_bytes(1, L) == ws
    check("switched to bf16x3", mid[0].cpu().numpy().T, reference(("tiny", L), sd, TINY, wav.cpu().numpy())["last_hidden_state"])
    m.set_precision("f32")
    after, _ = m(wav)
    assert torch.equal(before, after)


@pytest.mark.parametrize("precision", BOTH)
def test_large_widths_four_layers(precision):
    """conv 512 / hidden 1024 / 16 heads / FFN 4096: the real tile shapes, 16 heads in the attention's grid; 1 s (49 frames), 4 layers."""
    config = dict(LARGE, num_hidden_layers=4)
    m, sd = model_of("wide", config, precision)
    wav = O.synth_wav(SEED + 1, 16000)
    ref = reference("wide", sd, config, wav)
    out, frames = m(dev(wav))
    assert frames.tolist() == [49]
    check("wide last_hidden_state", out[0].cpu().numpy().T, ref["last_hidden_state"])
    check("wide hidden_states[2]", m(dev(wav), layer=2)[0][0].cpu().numpy().T, ref["hidden_states"][2])


@pytest.mark.parametrize("precision", BOTH)
def test_tiny_width_24_layers(precision):
    config = dict(TINY, num_hidden_layers=24)
    m, sd = model_of("deep", config, precision)
    wav = O.synth_wav(SEED + 2, 48000)
    out, _ = m(dev(wav))
    check("deep last_hidden_state", out[0].cpu().numpy().T, reference("deep", sd, config, wav)["last_hidden_state"])


@pytest.mark.parametrize("precision", BOTH)
def test_widths_of_the_32_deep_chunk(precision):
    """conv_dim 96 and intermediate_size 160 are no multiple of 64: those GEMMs stage 32-channel chunks, the window form (2 x 96) 64-channel ones."""
    config = dict(TINY, conv_dim=[96] * 7, intermediate_size=160)
    m, sd = model_of("odd", config, precision)
    wav = O.synth_wav(SEED + 5, samples(70))
    ref = reference("odd", sd, config, wav)
    feats = torch.full((1, 70, 96), float("nan"), device=DEV)
    m.debug_tap("extract_features", feats)
    try:
        out, _ = m(dev(wav))
    finally:
        m.debug_tap(None, None)
    check("odd extract_features", feats[0].cpu().numpy(), ref["extract_features"])
    check("odd last_hidden_state", out[0].cpu().numpy().T, ref["last_hidden_state"])


@pytest.mark.parametrize("precision", BOTH)
def test_conv_bias_false(precision):
    config = dict(TINY, conv_bias=False, mask_time_prob=0.0)
    m, sd = model_of("nobias", config, precision)
    wav = O.synth_wav(SEED + 3, samples(20))
    check("conv_bias=False", m(dev(wav))[0][0].cpu().numpy().T, reference("nobias", sd, config, wav)["last_hidden_state"])


def test_attention_with_logits_of_twelve():
    """bf16x3a on weights of gain 2: the logits reach +-12 (tests/hubert_bf16x3_emulation.py), so the softmax is no longer flat."""
    m, sd = model_of("gain2", TINY, "bf16x3a", gain=2.0)
    L = samples(65)
    wav = O.synth_wav(SEED + L, L)
    ref = O.forward(sd, TINY, wav)
    out, _ = m(dev(wav))
    check("gain 2 last_hidden_state", out[0].cpu().numpy().T, ref["last_hidden_state"])
    check("gain 2 hidden_states[1]", m(dev(wav), layer=1)[0][0].cpu().numpy().T, ref["hidden_states"][1])


@pytest.mark.parametrize("precision", BOTH)
def test_the_tap_that_exists_as_split_rows_only_is_refused_by_name(precision):
    m, _ = model_of("tiny", TINY, precision)
    with pytest.raises(RuntimeError, match=r"debug tap 'extractor\.0'.*split bf16"):
        m.debug_tap("extractor.0", torch.zeros((1, 80, 64), device=DEV))
    out, _ = m(dev(O.synth_wav(SEED, 800)))  # (the refused tap left nothing behind)
    assert out.shape == (1, 128, 2)


def test_predict_ema_end_to_end(tmp_path):
    """predict_ema --ssl-precision bf16x3a on a tiny HuBERT directory and four wavs of unequal length: the files equal
    HuBERT(precision="bf16x3a") -> forward_lowrate(interp_factor=4) composed by hand, and --batch-size 1 and 3 write identical bytes."""
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
        PE.main([str(d), str(wavs), str(tmp_path / f"out{bs}"), "--from-wav", "--ssl-model", str(hub), "--ssl-precision", "bf16x3a", "--batch-size", str(bs),
                 "--verbose", "0"])
    hubert = HuBERT.from_pretrained(str(hub), precision="bf16x3a").to(DEV)
    exact = HuBERT.from_pretrained(str(hub)).to(DEV)
    model = BiGRU(**params)
    model.load_state_dict(bsd)
    model = model.eval().to(DEV)
    differs = False
    for u, l in lens.items():
        y, _ = PE.read_wav(str(wavs / f"{u}.wav"))
        feats, frames = hubert(dev(y)[None])
        want = model.forward_lowrate(feats, lengths=frames, interp_factor=4)[0].T.cpu().numpy()
        a = np.load(tmp_path / "out1" / f"{u}.npy")
        assert a.shape == (4 * O.frames(l), 12) and a.dtype == np.float32
        assert np.array_equal(a, want), u
        assert (tmp_path / "out1" / f"{u}.npy").read_bytes() == (tmp_path / "out3" / f"{u}.npy").read_bytes(), u
        differs = differs or not torch.equal(feats, exact(dev(y)[None])[0])
    assert differs  # (the flag reached the encoder: the f32 model gives other bytes)
