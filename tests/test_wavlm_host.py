"""WavLM encoder, host side (no GPU): the float64 numpy oracle against the ``transformers`` library's golden (and the live library when it
imports), the bucket map against the library's, the sensitivity of the fixtures, the state_dict's key list, loading, the refusals, the C
ABI's new call without a device, and predict_ema's plan for a WavLM directory."""

import ctypes
import json
import os

import numpy as np
import pytest
import torch

from articulatory_amd import _native
from articulatory_amd.bin import predict_ema as PE
from articulatory_amd.features import HuBERT, WavLM, ssl_encoder_from_pretrained
from articulatory_amd.utils.synth import synth_hubert_state_dict, synth_wavlm_state_dict, wavlm_param_spec
from tests import wavlm_oracle as W
from tests.test_hubert_host import LARGE as HUBERT_LARGE, SEED, TINY as HUBERT_TINY, _model_dir, _write_wav

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (tools/make_golden_wavlm.py: TINY, LARGE) me = 8: exact buckets under 8, logarithmic ones for 8 .. 23, saturated from 24 on
TINY = dict(HUBERT_TINY, num_buckets=32, max_bucket_distance=24)
LARGE = dict(HUBERT_LARGE, num_buckets=320, max_bucket_distance=800)
GPU_TOL = 2e-5  # tests/test_gpu_wavlm.py


def samples(frames):
    return 400 + 320 * (frames - 1)


def test_oracle_reproduces_the_library_golden():
    gold = np.load(os.path.join(GOLDEN, "gold_wavlm.npz"))
    sd = synth_wavlm_state_dict(TINY, seed=SEED)
    lengths = sorted({int(k.split(".")[0][1:]) for k in gold.files})
    assert lengths == [samples(n) for n in (1, 2, 65, 129)]
    seen = 0
    for L in lengths:
        r = W.forward(sd, TINY, W.synth_wav(SEED + L, L))
        for key in (k for k in gold.files if k.startswith(f"L{L}.")):
            name = key.split(".", 1)[1]
            got = r["hidden_states"][int(name.rsplit(".", 1)[1])] if name.startswith("hidden_states.") else r[name]
            ref = gold[key]
            assert got.shape == ref.shape, key
            err = float(np.abs(got - ref).max() / np.abs(ref).max())
            assert err < 1e-10, (key, err)
            seen += 1
    assert seen == len(gold.files) == 3 * 4 + 1


def test_oracle_matches_the_live_library():
    pytest.importorskip("transformers")
    from tools.make_golden_wavlm import library_forward, library_model, load_synthetic

    model = library_model(TINY)
    sd = load_synthetic(model, TINY, seed=SEED + 1)
    L = samples(30)
    wav = W.synth_wav(SEED + L, L)
    r, ref = W.forward(sd, TINY, wav), library_forward(model, wav)
    for k, h in enumerate(ref.hidden_states):
        h = h[0].numpy()
        assert float(np.abs(r["hidden_states"][k] - h).max() / np.abs(h).max()) < 1e-10, k


@pytest.mark.parametrize("nb,md", [(32, 24), (320, 800), (64, 100)])
def test_bucket_map_is_the_librarys_for_every_distance(nb, md):
    pytest.importorskip("transformers")
    from transformers import WavLMConfig
    from transformers.models.wavlm.modeling_wavlm import WavLMAttention

    with torch.device("meta"):
        att = WavLMAttention(embed_dim=128, num_heads=2, num_buckets=nb, max_distance=md, has_relative_position_bias=True)
    table = _native.wavlm_bucket_of_distance(nb, md)
    assert table.dtype == torch.int32 and table.shape == (2 * md + 1,)
    d = torch.arange(-4000, 4001, dtype=torch.long)
    want = att._relative_positions_bucket(d)
    got = table[d.clamp(-md, md) + md].to(torch.long)  # (the kernel's clamp)
    assert torch.equal(got, want)
    assert int(table.min()) == 0 and int(table.max()) == nb - 1
    assert WavLMConfig().num_buckets == _native.WAVLM_DEFAULTS["num_buckets"] and WavLMConfig().max_bucket_distance == _native.WAVLM_DEFAULTS["max_bucket_distance"]


@pytest.mark.parametrize("T", [2, 30, 65, 129])
def test_fixtures_tell_a_wrong_bias_from_the_right_one(T):
    """Each change moves the last hidden state by more than 100 x the GPU tolerance.  One exception, which no weights can lift: at 2 frames
    every distance lies under the last exact bucket (8), so clamping there changes nothing at all — asserted as such."""
    sd = synth_wavlm_state_dict(TINY, seed=SEED)
    L = samples(T)
    wav = W.synth_wav(SEED + L, L)
    ref = W.forward(sd, TINY, wav)["last_hidden_state"]
    for v in W.VARIANTS:
        err = float(np.abs(W.forward(sd, TINY, wav, variant=v)["last_hidden_state"] - ref).max() / np.abs(ref).max())
        print(T, v, err)
        if v == "clamp_exact" and T - 1 <= TINY["num_buckets"] // 4:
            assert err == 0.0
        else:
            assert err > 100 * GPU_TOL, (T, v, err)


def test_state_dict_keys_are_the_library_models():
    with open(os.path.join(GOLDEN, "gold_wavlm_keys.txt")) as f:
        rows = [line.split() for line in f if line.strip()]
    for name, config in (("tiny", TINY), ("large", LARGE)):
        want = [(k, tuple(int(s) for s in shape.split(","))) for n, k, shape in rows if n == name]
        assert want and [(k, tuple(v)) for k, v in wavlm_param_spec(config).items()] == want
        with torch.device("meta"):
            m = WavLM(config)
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    m = WavLM(TINY)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v)) for k, v in wavlm_param_spec(TINY).items()]
    assert not m.training and m.config["num_buckets"] == 32
    assert _native.check_wavlm_config({})["max_bucket_distance"] == 800 and _native.check_wavlm_config({})["num_buckets"] == 320
    sd = synth_wavlm_state_dict(TINY, seed=1)
    assert all(v.dtype == np.float32 for v in sd.values())
    c = sd["encoder.layers.1.attention.gru_rel_pos_const"]
    assert 0.5 <= c.min() and c.max() <= 1.5 and np.abs(sd["encoder.layers.0.attention.rel_attn_embed.weight"]).max() > 1.5


def _wavlm_dir(path, safetensors=False, config=TINY):
    path.mkdir()
    (path / "config.json").write_text(json.dumps(dict(config, model_type="wavlm")))
    sd = {k: torch.from_numpy(v) for k, v in synth_wavlm_state_dict(config, seed=SEED).items()}
    if safetensors:
        from safetensors.torch import save_file

        save_file(sd, str(path / "model.safetensors"))
    else:
        torch.save(sd, path / "pytorch_model.bin")
    return path


def test_from_pretrained_and_dispatch(tmp_path):
    want = synth_wavlm_state_dict(TINY, seed=SEED)
    m = WavLM.from_pretrained(str(_wavlm_dir(tmp_path / "bin")))
    got = m.state_dict()
    assert list(got) == list(want) and all(np.array_equal(got[k].numpy(), want[k]) for k in want)
    native, rel = m.native_state(), m.rel_bias_state()
    assert sorted(rel) == sorted(k for k in want if "gru_rel_pos" in k or "rel_attn_embed" in k) and len(rel) == 1 + 3 * 2
    assert not set(native) & set(rel) and "encoder.pos_conv_embed.conv.weight_g" in native
    # the hand-over the first forward makes: every tensor is taken, in this order, and none is missing at finalize
    lib = _native.load_library()
    m._lib = lib
    h = ctypes.c_void_p()
    cfg = m._make_config()
    assert lib.hificar_hubert_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        for name, t in native.items():
            assert lib.hificar_hubert_set_weight(h, name.encode(), t.data_ptr(), (ctypes.c_int64 * t.dim())(*t.shape), t.dim()) == 0, name
        try:  # (without a device the upload fails — behind the check that every tensor arrived)
            m._finalize_handle(h)
        except RuntimeError as e:
            assert "Missing key" not in str(e) and "hificar_hubert_finalize" in str(e), e
    finally:
        lib.hificar_hubert_destroy(h)
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_state_dict({k: v for k, v in got.items() if k != "encoder.layers.1.attention.gru_rel_pos_linear.bias"})
    d = ssl_encoder_from_pretrained(str(tmp_path / "bin"), precision="bf16x3")
    assert type(d) is WavLM and d.precision == "bf16x3"
    hub = tmp_path / "hub"
    hub.mkdir()
    (hub / "config.json").write_text(json.dumps(dict(HUBERT_TINY, model_type="hubert")))
    torch.save({k: torch.from_numpy(v) for k, v in synth_hubert_state_dict(HUBERT_TINY, seed=SEED).items()}, hub / "pytorch_model.bin")
    assert type(ssl_encoder_from_pretrained(str(hub))) is HuBERT
    (hub / "config.json").write_text(json.dumps(dict(HUBERT_TINY, model_type="wav2vec2")))
    with pytest.raises(NotImplementedError, match="wav2vec2"):
        ssl_encoder_from_pretrained(str(hub))
    import pickle

    again = pickle.loads(pickle.dumps(d))
    assert type(again) is WavLM and again.precision == "bf16x3" and again._handle is None


def test_from_pretrained_safetensors(tmp_path):
    pytest.importorskip("safetensors")
    m = WavLM.from_pretrained(str(_wavlm_dir(tmp_path / "st", safetensors=True)))
    want = synth_wavlm_state_dict(TINY, seed=SEED)
    assert all(np.array_equal(m.state_dict()[k].numpy(), want[k]) for k in want)


def test_refusals():
    for bad, exc, text in (
            (dict(do_stable_layer_norm=False), NotImplementedError, r"WavLM: do_stable_layer_norm=False: post-LN encoders \(WavLM-base\)"),
            (dict(feat_extract_norm="group"), NotImplementedError, "WavLM.*group-norm extractors"),
            (dict(adapter_attn_dim=16), NotImplementedError, "WavLM.*adapters"),
            (dict(num_attention_heads=4), ValueError, "WavLM.*head size 64"),
            (dict(model_type="hubert"), NotImplementedError, "model_type 'hubert'"),
            (dict(num_buckets=31), ValueError, "num_buckets=31"),
            (dict(num_buckets=32, max_bucket_distance=8), ValueError, "max_bucket_distance=8")):
        with pytest.raises(exc, match=text):
            WavLM(dict(TINY, **bad))
    with pytest.raises(ValueError, match="WavLM: precision='bf16x3a' is not built"):
        WavLM(TINY, precision="bf16x3a")
    m = WavLM(TINY)
    with pytest.raises(ValueError, match="WavLM: precision='bf16x3a'"):
        m.set_precision("bf16x3a")
    with pytest.raises(NotImplementedError, match="WavLM: training"):
        m.train()
    with pytest.raises(RuntimeError, match="WavLM needs a CUDA/HIP tensor"):
        m(torch.zeros(1, 800))
    # HuBERT keeps refusing WavLM configurations, with the message it had
    with pytest.raises(NotImplementedError, match="WavLM's gated relative position bias is not built"):
        HuBERT(dict(TINY, model_type="wavlm"))
    with pytest.raises(NotImplementedError, match="WavLM's gated relative position bias is not built"):
        HuBERT(TINY)


def _handle(lib, config=HUBERT_TINY):
    h = ctypes.c_void_p()
    cfg = _native.make_hubert_config(_native.check_hubert_config(config), True, 1e-7)
    assert lib.hificar_hubert_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    return h


def _set(lib, h, name, shape):
    w = np.zeros(shape, dtype=np.float32)
    return lib.hificar_hubert_set_weight(h, name.encode(), w.ctypes.data, (ctypes.c_int64 * len(shape))(*shape), len(shape))


def test_c_abi_set_rel_bias_without_a_device():
    lib = _native.load_library()
    table = _native.wavlm_bucket_of_distance(32, 24)
    ptr = table.data_ptr()
    gate_w = "encoder.layers.1.attention.gru_rel_pos_linear.weight"
    h = _handle(lib)
    try:
        base = lib.hificar_hubert_workspace_bytes(h, 4, 16000)
        # without the call the names are unknown, as ever
        assert _set(lib, h, gate_w, (8, 64)) == _native.E_INVALID and b"unexpected tensor name" in lib.hificar_last_error()
        assert _set(lib, h, "encoder.layers.0.attention.rel_attn_embed.weight", (32, 2)) == _native.E_INVALID
        for nb, md in ((31, 24), (0, 24), (-2, 24), (32, 0), (32, -1)):
            assert lib.hificar_hubert_set_rel_bias(h, nb, md, ptr) == _native.E_INVALID, (nb, md)
        assert lib.hificar_hubert_set_rel_bias(h, 32, 24, None) == _native.E_INVALID
        bad = table.clone()
        bad[5] = 32
        assert lib.hificar_hubert_set_rel_bias(h, 32, 24, bad.data_ptr()) == _native.E_INVALID and b"bucket_of_distance[5]=32" in lib.hificar_last_error()
        bad[5] = -1
        assert lib.hificar_hubert_set_rel_bias(h, 32, 24, bad.data_ptr()) == _native.E_INVALID
        assert _set(lib, h, gate_w, (8, 64)) == _native.E_INVALID  # (a refused call switched nothing on)
        assert lib.hificar_hubert_set_rel_bias(h, 32, 24, ptr) == 0
        assert _set(lib, h, gate_w, (8, 64)) == 0
        assert _set(lib, h, gate_w, (64, 8)) == _native.E_INVALID and b"size mismatch" in lib.hificar_last_error()
        assert _set(lib, h, "encoder.layers.0.attention.gru_rel_pos_linear.bias", (8,)) == 0
        assert _set(lib, h, "encoder.layers.0.attention.gru_rel_pos_const", (1, 2, 1, 1)) == 0
        assert _set(lib, h, "encoder.layers.0.attention.gru_rel_pos_const", (2,)) == _native.E_INVALID
        assert _set(lib, h, "encoder.layers.0.attention.rel_attn_embed.weight", (32, 2)) == 0
        assert _set(lib, h, "encoder.layers.0.attention.rel_attn_embed.weight", (2, 32)) == _native.E_INVALID
        assert _set(lib, h, "encoder.layers.1.attention.rel_attn_embed.weight", (32, 2)) == _native.E_INVALID  # (layer 0 owns the table)
        # the workspace grows by one layer's gates only: B heads Tmax floats (256-byte granules)
        grown = lib.hificar_hubert_workspace_bytes(h, 4, 16000) - base
        assert 4 * 2 * 49 * 4 <= grown < 4 * 2 * 49 * 4 + 256
        # bf16x3a after the call; bf16x3 is taken
        assert lib.hificar_hubert_set_precision(h, _native.PREC_BF16X3A) == _native.E_INVALID and b"bf16x3a" in lib.hificar_last_error()
        assert lib.hificar_hubert_set_precision(h, _native.PREC_BF16X3) == 0
        assert lib.hificar_hubert_finalize(h) == _native.E_STATE and b"Missing key" in lib.hificar_last_error()
    finally:
        lib.hificar_hubert_destroy(h)
    h = _handle(lib)
    try:  # ... and the call on a bf16x3a handle
        assert lib.hificar_hubert_set_precision(h, _native.PREC_BF16X3A) == 0
        assert lib.hificar_hubert_set_rel_bias(h, 32, 24, ptr) == _native.E_INVALID and b"bf16x3a" in lib.hificar_last_error()
        assert _set(lib, h, gate_w, (8, 64)) == _native.E_INVALID
    finally:
        lib.hificar_hubert_destroy(h)
    # the large model: 6404 bytes of table per head, B heads Tmax floats of gates
    h = _handle(lib, HUBERT_LARGE)
    try:
        base = lib.hificar_hubert_workspace_bytes(h, 64, 160000)
        big = _native.wavlm_bucket_of_distance(320, 800)
        assert 4 * big.numel() == 6404 and lib.hificar_hubert_set_rel_bias(h, 320, 800, big.data_ptr()) == 0
        grown = lib.hificar_hubert_workspace_bytes(h, 64, 160000) - base
        assert 64 * 16 * 499 * 4 <= grown < 64 * 16 * 499 * 4 + 256
    finally:
        lib.hificar_hubert_destroy(h)


def test_predict_ema_plan_for_a_wavlm_directory(tmp_path, capsys):
    d = _model_dir(tmp_path, "foo_h2")
    wl = tmp_path / "wavlm"
    wl.mkdir()
    (wl / "config.json").write_text(json.dumps(dict(TINY, model_type="wavlm")))  # (no weights: the plan reads the configuration alone)
    wavs = tmp_path / "wavs"
    wavs.mkdir()
    _write_wav(wavs / "a.wav", 16000)

    def plan(*extra):
        PE.main([str(d), str(wavs), str(tmp_path / "never"), "--dry-run", "--verbose", "0", "--from-wav", "--ssl-model", str(wl), *extra])
        return json.loads(capsys.readouterr().out)

    p = plan("--ssl-layer", "1", "--ssl-precision", "bf16x3")
    assert (p["front_end"], p["ssl_layer"], p["ssl_precision"], p["frames"], p["hidden_size"]) == ("wavlm", 1, "bf16x3", 49, 128)
    with pytest.raises(ValueError, match="WavLM: precision='bf16x3a' is not built"):
        plan("--ssl-precision", "bf16x3a")
    (wl / "config.json").write_text(json.dumps(dict(TINY, model_type="wavlm", do_stable_layer_norm=False)))
    with pytest.raises(NotImplementedError, match="WavLM.*post-LN"):
        plan()
