"""HuBERT encoder, host side (no GPU): the float64 numpy oracle against the ``transformers`` library's golden, the frame rule, the
state_dict's key list, ``from_pretrained``, every refusal, and predict_ema's ``--ssl-model`` plan."""

import ctypes
import json
import os
import wave

import numpy as np
import pytest
import torch
import yaml

from articulatory_amd import _native
from articulatory_amd.bin import predict_ema as PE
from articulatory_amd.features import HuBERT
from articulatory_amd.utils.synth import hubert_param_spec, synth_bigru_state_dict, synth_hubert_state_dict
from tests import hubert_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (tools/make_golden_hubert.py: TINY, LARGE, SEED)
TINY = dict(conv_dim=[64] * 7, conv_kernel=list(O.KERNELS), conv_stride=list(O.STRIDES), hidden_size=128, num_attention_heads=2, intermediate_size=256,
            num_hidden_layers=2, conv_bias=True, feat_extract_norm="layer", do_stable_layer_norm=True, feat_proj_layer_norm=True,
            layer_norm_eps=1e-5, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, hidden_act="gelu",
            feat_extract_activation="gelu", mask_time_prob=0.05, mask_feature_prob=0.0)
LARGE = dict(TINY, conv_dim=[512] * 7, hidden_size=1024, num_attention_heads=16, intermediate_size=4096, num_hidden_layers=24)
SEED = 4242


def test_oracle_reproduces_the_library_golden():
    gold = np.load(os.path.join(GOLDEN, "gold_hubert.npz"))
    sd = synth_hubert_state_dict(TINY, seed=SEED)
    lengths = sorted({int(k.split(".")[0][1:]) for k in gold.files})
    assert lengths == [400, 719, 720, 20880, 41360]
    seen = 0
    for L in lengths:
        r = O.forward(sd, TINY, O.synth_wav(SEED + L, L))
        for key in (k for k in gold.files if k.startswith(f"L{L}.")):
            name = key.split(".", 1)[1]
            got = r["hidden_states"][int(name.rsplit(".", 1)[1])] if name.startswith("hidden_states.") else r[name]
            ref = gold[key]
            assert got.shape == ref.shape, key
            err = float(np.abs(got - ref).max() / np.abs(ref).max())
            assert err < 1e-9, (key, err)
            seen += 1
    assert seen == len(gold.files) == 4 * 6 + 3 + 1


def test_frames_rule():
    lib = _native.load_library()
    with pytest.raises(ValueError, match="under 400 samples"):
        HuBERT.frames(399)
    assert lib.hificar_hubert_frames(None, 399) == 0 and O.frames(399) == 0
    for L, n in ((400, 1), (719, 1), (720, 2), (16000, 49)):
        assert HuBERT.frames(L) == n and lib.hificar_hubert_frames(None, L) == n and O.frames(L) == n
        x = np.zeros((L, 1))
        for k, s in zip(O.KERNELS, O.STRIDES):  # the seven convs' lengths composed
            x = x[: (x.shape[0] - k) // s + 1]
        assert x.shape[0] == n


def test_state_dict_keys_are_the_library_models():
    with open(os.path.join(GOLDEN, "gold_hubert_keys.txt")) as f:
        rows = [line.split() for line in f if line.strip()]
    for name, config in (("tiny", TINY), ("large", LARGE)):
        want = [(k, tuple(int(s) for s in shape.split(","))) for n, k, shape in rows if n == name]
        assert want and [(k, tuple(v)) for k, v in hubert_param_spec(config).items()] == want
    one_wide = dict(LARGE, num_hidden_layers=1)
    for config in (TINY, one_wide, dict(TINY, conv_bias=False, mask_time_prob=0.0)):
        m = HuBERT(config)
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v)) for k, v in hubert_param_spec(config).items()]
        assert not m.training
    sd = synth_hubert_state_dict(TINY, seed=1)
    assert all(v.dtype == np.float32 for v in sd.values())
    ln = [k for k in sd if "layer_norm" in k]
    assert all(np.abs(sd[k] - 1).max() > 0.1 for k in ln if k.endswith("weight")) and all(np.abs(sd[k]).max() > 0.1 for k in ln if k.endswith("bias"))


def _old_form(sd):
    p = "encoder.pos_conv_embed.conv."
    return {k.replace(p + "parametrizations.weight.original0", p + "weight_g").replace(p + "parametrizations.weight.original1", p + "weight_v"): v
            for k, v in sd.items()}


def _hubert_dir(path, config=TINY, seed=SEED, old_form=False, safetensors=False):
    path.mkdir()
    (path / "config.json").write_text(json.dumps(dict(config, model_type="hubert")))
    sd = {k: torch.from_numpy(v) for k, v in synth_hubert_state_dict(config, seed=seed).items()}
    if old_form:
        sd = _old_form(sd)
    if safetensors:
        from safetensors.torch import save_file

        save_file(sd, str(path / "model.safetensors"))
    else:
        torch.save(sd, path / "pytorch_model.bin")
    return path


@pytest.mark.parametrize("old_form", [False, True])
def test_from_pretrained_round_trip(tmp_path, old_form):
    m = HuBERT.from_pretrained(str(_hubert_dir(tmp_path / "hub", old_form=old_form)))
    want = synth_hubert_state_dict(TINY, seed=SEED)
    got = m.state_dict()
    assert list(got) == list(want) and all(np.array_equal(got[k].numpy(), want[k]) for k in want)
    native = m.native_state()
    assert "masked_spec_embed" not in native and "encoder.pos_conv_embed.conv.weight_g" in native and "encoder.pos_conv_embed.conv.weight_v" in native
    assert not any("parametrizations" in k for k in native)
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_state_dict({k: v for k, v in got.items() if k != "encoder.layer_norm.bias"})
    with pytest.raises(RuntimeError, match="Unexpected key"):
        m.load_state_dict(dict(got, extra=torch.zeros(1)))


def test_from_pretrained_safetensors_and_foreign_layouts(tmp_path):
    pytest.importorskip("safetensors")
    m = HuBERT.from_pretrained(str(_hubert_dir(tmp_path / "st", safetensors=True)))
    want = synth_hubert_state_dict(TINY, seed=SEED)
    assert all(np.array_equal(m.state_dict()[k].numpy(), want[k]) for k in want)
    d = tmp_path / "fairseq"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(TINY))
    torch.save({"model": {"encoder.layers.0.self_attn.k_proj.weight": torch.zeros(2, 2)}, "cfg": {}}, d / "pytorch_model.bin")
    with pytest.raises(NotImplementedError, match="fairseq / s3prl"):
        HuBERT.from_pretrained(str(d))
    torch.save({"encoder.layers.0.self_attn.k_proj.weight": torch.zeros(2, 2)}, d / "pytorch_model.bin")
    with pytest.raises(NotImplementedError, match="fairseq / s3prl"):
        HuBERT.from_pretrained(str(d))


def test_refusals():
    for bad, exc, text in (
            (dict(feat_extract_norm="group"), NotImplementedError, "group-norm extractors"),
            (dict(do_stable_layer_norm=False), NotImplementedError, "post-LN"),
            (dict(feat_proj_layer_norm=False), NotImplementedError, "feat_proj_layer_norm"),
            (dict(model_type="wavlm"), NotImplementedError, "gated relative position bias"),
            (dict(num_buckets=320), NotImplementedError, "gated relative position bias"),
            (dict(hidden_act="relu"), NotImplementedError, "gelu"),
            (dict(conv_kernel=[10, 3, 3, 3, 3, 3, 2]), NotImplementedError, "conv_kernel"),
            (dict(num_conv_pos_embeddings=127), NotImplementedError, "positional conv"),
            (dict(adapter_attn_dim=16), NotImplementedError, "adapters"),
            (dict(conv_dim=[64] * 6 + [128]), NotImplementedError, "one width"),
            (dict(num_attention_heads=4), ValueError, "head size 64"),
            (dict(hidden_size=192, num_attention_heads=3), ValueError, "hidden_size=192"),
            (dict(conv_dim=[48] * 7), ValueError, "conv_dim=48"),
            (dict(intermediate_size=100), ValueError, "intermediate_size"),
            (dict(num_hidden_layers=0), ValueError, "num_hidden_layers")):
        with pytest.raises(exc, match=text):
            HuBERT(dict(TINY, **bad))
    m = HuBERT(TINY)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.train()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 800))
    with pytest.raises(NotImplementedError, match="front end"):
        m.forward_lowrate(torch.zeros(1, 128, 4))
    assert m.eval() is m


def test_c_abi_refusals_without_a_device():
    lib = _native.load_library()
    h = ctypes.c_void_p()
    cfg = _native.make_hubert_config(_native.check_hubert_config(TINY), True, 1e-7)
    cfg.hidden_size = 192
    assert lib.hificar_hubert_create(ctypes.byref(cfg), ctypes.byref(h)) == _native.E_INVALID
    assert b"hidden_size=192" in lib.hificar_last_error()
    cfg.hidden_size, cfg.num_attention_heads = 128, 4
    assert lib.hificar_hubert_create(ctypes.byref(cfg), ctypes.byref(h)) == _native.E_INVALID
    assert b"head size 64" in lib.hificar_last_error()
    cfg.num_attention_heads = 2
    assert lib.hificar_hubert_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        w = np.zeros((128,), dtype=np.float32)
        shape = (ctypes.c_int64 * 1)(128)
        assert lib.hificar_hubert_set_weight(h, b"encoder.layer_norm.weight", w.ctypes.data, shape, 1) == 0
        assert lib.hificar_hubert_set_weight(h, b"encoder.nope", w.ctypes.data, shape, 1) == _native.E_INVALID
        shape[0] = 64
        assert lib.hificar_hubert_set_weight(h, b"encoder.layer_norm.bias", w.ctypes.data, shape, 1) == _native.E_INVALID
        assert b"size mismatch" in lib.hificar_last_error()
        assert lib.hificar_hubert_finalize(h) == _native.E_STATE and b"Missing key" in lib.hificar_last_error()
        assert lib.hificar_hubert_workspace_bytes(h, 1, 399) == 0 and lib.hificar_hubert_workspace_bytes(h, 0, 16000) == 0
        assert lib.hificar_hubert_workspace_bytes(h, 4, 16000) > 0
        assert lib.hificar_hubert_forward(h, 256, None, None, 256, 1, 399, -1, 256, 1 << 40, None) == _native.E_INVALID
        assert lib.hificar_hubert_forward(h, 256, None, None, 256, 1, 800, 2, 256, 1 << 40, None) == _native.E_INVALID and b"layer=2" in lib.hificar_last_error()
        assert lib.hificar_hubert_forward(h, 256, None, None, 256, 1, 800, -1, 256, 1 << 40, None) == _native.E_STATE
    finally:
        lib.hificar_hubert_destroy(h)
    # the large model at B = 64 x 10 s: the extractor runs over sub-batches, so the workspace stays far below the 4.2 GB that layer 0's rows
    # of the whole batch would take, and grows with B by the 50-Hz rows only
    cfg = _native.make_hubert_config(_native.check_hubert_config(LARGE), True, 1e-7)
    assert lib.hificar_hubert_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        n64, n8 = lib.hificar_hubert_workspace_bytes(h, 64, 160000), lib.hificar_hubert_workspace_bytes(h, 8, 160000)
        per_frame = 4 * (512 + 4 * 1024 + 4096)
        assert 0 < n8 < n64 < 2 * 2 ** 30
        assert abs((n64 - n8) - 56 * 499 * per_frame) <= 256 * per_frame
    finally:
        lib.hificar_hubert_destroy(h)


def _write_wav(path, n, rate=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes((np.arange(n) % 200 - 100).astype("<i2").tobytes())


def _model_dir(tmp_path, name, in_channels=128):
    d = tmp_path / name
    d.mkdir()
    params = dict(in_channels=in_channels, hidden_size=64, out_channels=12, use_tanh=False)
    (d / "config.yml").write_text(yaml.safe_dump({"generator_type": "BiGRU", "generator_params": params}))
    sd = synth_bigru_state_dict(params, seed=3)
    torch.save({"model": {"generator": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}}, d / PE.CHECKPOINT)
    return d


def test_predict_ema_ssl_plan_and_errors(tmp_path, capsys):
    d = _model_dir(tmp_path, "foo_h2")
    hub = tmp_path / "hub"
    hub.mkdir()
    (hub / "config.json").write_text(json.dumps(TINY))  # (no weights: the plan reads the configuration alone)
    wavs = tmp_path / "wavs"
    wavs.mkdir()
    _write_wav(wavs / "a.wav", 16000)
    _write_wav(wavs / "b.wav", 719)

    def plan(*extra, model=d):
        PE.main([str(model), str(wavs), str(tmp_path / "never"), "--dry-run", "--verbose", "0", *extra])
        return json.loads(capsys.readouterr().out)

    p = plan("--from-wav", "--ssl-model", str(hub), "--batch-size", "3")
    assert (p["front_end"], p["ssl_model"], p["ssl_layer"], p["frames"], p["samples"]) == ("hubert", str(hub), -1, 49 + 1, 16719)
    assert (p["interp_factor"], p["zscore"], p["batch_size"], p["utterances"], p["hidden_size"]) == (4, False, 3, ["a", "b"], 128)
    assert plan("--from-wav", "--ssl-model", str(hub), "--ssl-layer", "1")["ssl_layer"] == 1
    assert not (tmp_path / "never").exists()
    with pytest.raises(NotImplementedError, match="SSL extraction is not built.*--ssl-model"):
        plan("--from-wav")
    with pytest.raises(ValueError, match="--ssl-layer 2 outside"):
        plan("--from-wav", "--ssl-model", str(hub), "--ssl-layer", "2")
    with pytest.raises(ValueError, match="--ssl-layer belongs"):
        plan("--from-wav", "--ssl-layer", "1", model=_model_dir(tmp_path, "foo_mfcc", 13))
    with pytest.raises(ValueError, match="--ssl-model belongs"):
        plan("--from-wav", "--ssl-model", str(hub), model=tmp_path / "foo_mfcc")
    with pytest.raises(ValueError, match="--ssl-model belongs"):
        plan("--ssl-model", str(hub))
    with pytest.raises(ValueError, match="--hop-length belongs"):
        plan("--from-wav", "--ssl-model", str(hub), "--hop-length", "80")
    _write_wav(wavs / "c.wav", 399)
    with pytest.raises(ValueError, match=r"c\.wav: 399 samples"):
        plan("--from-wav", "--ssl-model", str(hub))
    os.remove(wavs / "c.wav")
    _write_wav(wavs / "d.wav", 8000, rate=8000)
    with pytest.raises(ValueError, match=r"d\.wav: sampling rate 8000"):
        plan("--from-wav", "--ssl-model", str(hub))
    (hub / "config.json").write_text(json.dumps(dict(TINY, feat_extract_norm="group")))
    with pytest.raises(NotImplementedError, match="group-norm"):
        plan("--from-wav", "--ssl-model", str(hub))
