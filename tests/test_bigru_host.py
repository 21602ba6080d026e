"""The BiGRU inversion model's host side (reference articulatory/models/pytorch_models.py:22-123): state_dict surface, loading, the CPU
restatement the GPU tests measure against, refusals, the C struct, and the ``art`` decode path.  No GPU."""

import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from bigru_oracle import BiGRUOracle
from conftest import GOLDEN, REPO, rel_err
from articulatory_amd import _native
from articulatory_amd.bin import decode as D
from articulatory_amd.models import BiGRU
from articulatory_amd.utils import load_model
from articulatory_amd.utils.synth import bigru_param_spec, synth_bigru_state_dict, uniform

CASES = {"full": (400,), "mfcc": (500,), "small": (1, 300)}


def gold():
    return np.load(os.path.join(GOLDEN, "gold_bigru.npz"))


def case_params(g, tag):
    cin, hidden, out, tanh, seed = (int(v) for v in g[tag + "_params"])
    return dict(in_channels=cin, hidden_size=hidden, out_channels=out, use_tanh=bool(tanh)), seed


def case_input(g, tag, T):
    """The stored input of a case; the (1024, 256, 18) one is regenerated as tools/make_golden_bigru.py drew it (too large to commit)."""
    key = f"{tag}_T{T}_x"
    if key in g:
        return g[key]
    params, seed = case_params(g, tag)
    return uniform(seed, f"x.{T}", (1, params["in_channels"], T), -1.0, 1.0)


def torch_sd(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def test_state_dict_keys_shapes_and_order():
    g = gold()
    params, _ = case_params(g, "full")
    want = open(os.path.join(GOLDEN, "gold_bigru_keys.txt")).read().split()
    sd = BiGRU(**params).state_dict()
    assert list(sd.keys()) == want == list(bigru_param_spec(**params).keys())
    for k, shape in bigru_param_spec(**params).items():
        assert tuple(sd[k].shape) == tuple(shape), k
    assert sd["bn.num_batches_tracked"].dtype == torch.int64
    assert sd["gru1.weight_ih_l0_reverse"].shape == (768, 1024) and sd["gru2.weight_ih_l0"].shape == (768, 512)
    tanh = BiGRU(in_channels=13, hidden_size=64, out_channels=12, use_tanh=True).state_dict()
    assert list(tanh.keys())[-2:] == ["fc2.0.weight", "fc2.0.bias"]
    # constructor keywords and defaults of the reference (pytorch_models.py:23-25)
    import inspect
    sig = inspect.signature(BiGRU.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [
        ("in_channels", 80), ("hidden_size", 256), ("dropout", 0.3), ("out_channels", 1), ("use_ar", False), ("ar_input", 512),
        ("ar_hidden", 256), ("ar_output", 128), ("ar_channels", None), ("use_tanh", False), ("use_spk_emb", False), ("spk_emb_size", 32),
        ("spk_emb_hidden", 32)]
    assert list(inspect.signature(BiGRU.forward).parameters)[1:] == ["mels", "mask", "spk_id", "spk", "ar", "ph", "lengths"]
    assert inspect.signature(BiGRU.inference).parameters["normalize_before"].default is True


def test_reference_layout_checkpoint_loads_strict(tmp_path):
    params = dict(in_channels=80, hidden_size=64, out_channels=12, use_tanh=False)
    sd = synth_bigru_state_dict(params, seed=7)
    m = BiGRU(**params)
    res = m.load_state_dict(torch_sd(sd), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), sd[k]), k
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_state_dict({k: v for k, v in torch_sd(sd).items() if k != "bn.running_var"}, strict=True)
    # load_model: the out_channels > 1 refusal is for the waveform generators only; stats.npy beside the checkpoint is picked up
    torch.save({"model": {"generator": torch_sd(sd)}}, tmp_path / "checkpoint-1steps.pkl")
    config = dict(generator_type="BiGRU", generator_params=params, format="npy")
    stats = np.stack([np.linspace(-1, 1, 80), np.linspace(0.5, 2, 80)]).astype(np.float32)
    np.save(tmp_path / "stats.npy", stats)
    model = load_model(str(tmp_path / "checkpoint-1steps.pkl"), config)
    assert isinstance(model, BiGRU) and not hasattr(model, "pqmf")
    assert np.array_equal(model.mean.numpy(), stats[0]) and np.array_equal(model.scale.numpy(), stats[1])
    model.remove_weight_norm()  # exists, changes nothing
    assert list(model.state_dict().keys()) == ["mean", "scale"] + list(sd.keys())  # (the reference's module lists its own buffers first too)


def test_restatement_matches_the_reference_goldens():
    """tests/bigru_oracle.py against every case of the real reference class, within 4 x the case's recorded fp32-vs-float64 deviation (two
    fp32 evaluations of one function are each ``dev`` from float64; the other factor 2 allows for another thread count or SIMD path).
    Measured here (8 threads): 0 for every case — the restatement runs the reference's own operators — against recorded deviations of
    4.3e-7 (full_T400), 5.2e-7 (mfcc_T500), 1.4e-7 (small_T1), 5.7e-7 (small_T300), 3.3e-7 / 4.3e-7 (inference), 3.5e-7 (ragged)."""
    g = gold()
    for tag, frames in CASES.items():
        params, seed = case_params(g, tag)
        o = BiGRUOracle(synth_bigru_state_dict(params, seed=seed), use_tanh=params["use_tanh"])
        for T in frames:
            y = o.forward(case_input(g, tag, T)).numpy()
            err, dev = rel_err(y, g[f"{tag}_T{T}_y"]), float(g[f"{tag}_T{T}_f32_dev"])
            print(f"{tag}_T{T}: restatement vs golden {err:.3g}, recorded f32 dev {dev:.3g}")
            assert dev <= 2e-6 and err <= 4 * dev
        if tag == "small":
            o.register_stats(g["small_stats"][0], g["small_stats"][1])
            for key, nb in (("small_inf", True), ("small_inf_raw", False)):
                err = rel_err(o.inference(g["small_inf_c"], normalize_before=nb).numpy(), g[key + "_y"])
                print(f"{key}: {err:.3g}")
                assert err <= 4 * float(g[key + "_f32_dev"])
            yr = o.forward(g["small_ragged_x"], lengths=[int(v) for v in g["small_ragged_lengths"]]).numpy()
            assert rel_err(yr, g["small_ragged_y"]) <= 4 * float(g["small_ragged_f32_dev"])


def test_ragged_restatement_equals_alone_bitwise():
    g = gold()
    params, seed = case_params(g, "small")
    o = BiGRUOracle(synth_bigru_state_dict(params, seed=seed))
    x, lens = g["small_ragged_x"], [int(v) for v in g["small_ragged_lengths"]]
    y = o.forward(x, lengths=lens)
    for b, n in enumerate(lens):
        assert torch.equal(y[b, :, :n], o.forward(x[b:b + 1, :, :n])[0]) and not y[b, :, n:].any()
    # zero padding is NOT the same thing: the reverse direction would start in the padding
    assert not torch.equal(o.forward(x[1:2])[0, :, :1], y[1, :, :1])


def test_refusals():
    with pytest.raises(NotImplementedError, match="use_ar"):
        BiGRU(use_ar=True)
    with pytest.raises(NotImplementedError, match="use_spk_emb"):
        BiGRU(use_spk_emb=True)
    with pytest.raises(ValueError, match="hidden_size"):
        BiGRU(hidden_size=100)
    with pytest.raises(ValueError, match="hidden_size"):
        BiGRU(hidden_size=512)
    with pytest.raises(ValueError, match="out_channels"):
        BiGRU(out_channels=64)
    for params in ((1024, 256, 18), (13, 256, 12), (80, 64, 12)):  # the goldens' shapes are inside the engine's limits
        _native.check_bigru_params(dict(in_channels=params[0], hidden_size=params[1], out_channels=params[2]))
    m = BiGRU(in_channels=13, hidden_size=64, out_channels=12)
    x = torch.zeros(1, 13, 5)
    with pytest.raises(NotImplementedError, match=r"train\(\) mode"):
        m(x)
    m.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.inference(np.zeros((5, 13), dtype=np.float32), normalize_before=False)
    # training stays out of scope: the trainer refuses the type
    from articulatory_amd.bin.train import Trainer
    with pytest.raises(NotImplementedError, match="BiGRU"):
        Trainer(dict(generator_type="BiGRU"), "cpu")


def test_config_struct_matches_header_and_create_checks():
    assert ctypes.sizeof(_native.HificarBigruConfig) == 16
    hdr = open(os.path.join(REPO, "include", "hificar.h")).read()
    for name, v in (("IN", _native.BIGRU_MAX_IN), ("HIDDEN", _native.BIGRU_MAX_HIDDEN), ("OUT", _native.BIGRU_MAX_OUT)):
        assert f"#define HIFICAR_BIGRU_MAX_{name} {v}" in hdr
    lib = _native.load_library()
    h = ctypes.c_void_p()
    cfg = _native.make_bigru_config(dict(in_channels=80, hidden_size=64, out_channels=12, use_tanh=True))
    _native.check(lib.hificar_bigru_create(ctypes.byref(cfg), ctypes.byref(h)), "hificar_bigru_create")
    try:
        # pre-gates B T 6H floats + rows B T max(96, 2H) floats, B T rounded up to 256 rows
        assert lib.hificar_bigru_workspace_bytes(h, 2, 300) == 768 * (6 * 64 + 128) * 4
        w = np.zeros((12, 128), dtype=np.float32)
        shape = (ctypes.c_int64 * 2)(12, 128)
        assert lib.hificar_bigru_set_weight(h, b"fc2.0.weight", w.ctypes.data, shape, 2) == 0
        assert lib.hificar_bigru_set_weight(h, b"fc2.weight", w.ctypes.data, shape, 2) == -1
        assert b"unexpected tensor name" in lib.hificar_last_error()
        shape = (ctypes.c_int64 * 2)(128, 12)
        assert lib.hificar_bigru_set_weight(h, b"fc2.0.weight", w.ctypes.data, shape, 2) == -1
        assert b"size mismatch" in lib.hificar_last_error()
        assert lib.hificar_bigru_finalize(h) == -2 and b"Missing key" in lib.hificar_last_error()
    finally:
        lib.hificar_bigru_destroy(h)
    bad = _native.make_bigru_config(dict(in_channels=80, hidden_size=96, out_channels=12, use_tanh=False))
    assert lib.hificar_bigru_create(ctypes.byref(bad), ctypes.byref(h)) == -1 and b"hidden_size" in lib.hificar_last_error()


class _StubInversion:
    """Stands in for the device model in the decode loop: (T, C) -> (T, out) by the CPU restatement."""

    def __init__(self, oracle):
        self.o = oracle
        self.mean, self.scale = oracle.mean, oracle.scale
        self.calls = []

    def inference(self, c, normalize_before=True):
        self.calls.append(("inference", tuple(c.shape), normalize_before))
        return self.o.inference(c, normalize_before=normalize_before)

    def __call__(self, x, lengths=None):
        self.calls.append(("forward", tuple(x.shape), list(lengths)))
        return self.o.forward(x, lengths=lengths)


def _dump(tmp_path, g):
    dump = tmp_path / "dump"
    dump.mkdir()
    feats = {"uttA": g["small_inf_c"], "uttB": g["small_inf_c"][:77].copy(), "uttC": g["small_inf_c"][40:41].copy()}
    for u, c in feats.items():
        np.save(dump / f"{u}-feats.npy", c)
    scp = tmp_path / "feats.scp"
    scp.write_text("".join(f"{u} {dump / (u + '-feats.npy')}\n" for u in feats))
    return dump, scp, feats


def test_decode_art_mode_writes_gen_npy(tmp_path):
    g = gold()
    params, seed = case_params(g, "small")
    o = BiGRUOracle(synth_bigru_state_dict(params, seed=seed))
    o.register_stats(g["small_stats"][0], g["small_stats"][1])
    dump, scp, feats = _dump(tmp_path, g)
    config = dict(generator_params=params, dataset_mode="art")
    for kw, sub in ((dict(feats_scp=str(scp)), "out_scp"), (dict(dumpdir=str(dump)), "out_dump")):
        out = tmp_path / sub
        out.mkdir()
        model = _StubInversion(o)
        n, sec = D.decode_features(model, D.iter_features(**kw), config, "cpu", str(out), normalize_before=True)
        assert n == 3 and sec > 0 and [c[0] for c in model.calls] == ["inference"] * 3
        y = np.load(out / "uttA_gen.npy")
        assert y.shape == (200, 12) and y.dtype == np.float32 and rel_err(y, g["small_inf_y"]) <= 4 * float(g["small_inf_f32_dev"])
        assert np.load(out / "uttB_gen.npy").shape == (77, 12) and np.load(out / "uttC_gen.npy").shape == (1, 12)
        # ragged batches: the same files
        outb = tmp_path / (sub + "_b4")
        outb.mkdir()
        model = _StubInversion(o)
        n, _ = D.decode_features(model, D.iter_features(**kw), config, "cpu", str(outb), normalize_before=True, batch_size=4)
        assert n == 3 and model.calls == [("forward", (3, 80, 200), [1, 77, 200])]
        for u in feats:
            assert np.array_equal(np.load(outb / f"{u}_gen.npy"), np.load(out / f"{u}_gen.npy")), u
    raw = tmp_path / "raw"
    raw.mkdir()
    D.decode_features(_StubInversion(o), D.iter_features(feats_scp=str(scp)), config, "cpu", str(raw), normalize_before=False)
    assert rel_err(np.load(raw / "uttA_gen.npy"), g["small_inf_raw_y"]) <= 4 * float(g["small_inf_raw_f32_dev"])


def test_decode_cli_modes(tmp_path):
    """--dry-run in ``art`` mode (no GPU, no checkpoint read); ``w2a`` and an AR model in ``art`` mode stay refused."""
    g = gold()
    params, _ = case_params(g, "small")
    dump, scp, feats = _dump(tmp_path, g)
    cfg = tmp_path / "config.yml"
    cfg.write_text(yaml.safe_dump(dict(generator_type="BiGRU", generator_params=params, dataset_mode="art", format="npy")))
    env = dict(os.environ, PYTHONPATH=REPO)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "articulatory_amd.bin.decode", "--feats-scp", str(scp), "--outdir", str(tmp_path / "o"),
                        "--checkpoint", str(tmp_path / "none.pkl"), "--config", str(cfg), "--dry-run"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["utterances"] == list(feats) and info["frames"] == 278 and info["world_size"] == 1
    args = ["--feats-scp", str(scp), "--outdir", str(tmp_path / "o"), "--checkpoint", str(tmp_path / "none.pkl"), "--dry-run"]
    for mode in ("w2a", "ph2m", "ph2a", "a2w_mult"):
        bad = tmp_path / f"{mode}.yml"
        bad.write_text(yaml.safe_dump(dict(generator_type="BiGRU", generator_params=params, dataset_mode=mode, format="npy")))
        with pytest.raises(NotImplementedError, match=mode):
            D.main(args + ["--config", str(bad)])
    ar = tmp_path / "ar.yml"
    ar.write_text(yaml.safe_dump(dict(generator_type="HiFiGANGenerator", generator_params=dict(use_ar=True), dataset_mode="art", format="npy")))
    with pytest.raises(NotImplementedError, match="use_ar"):
        D.main(args + ["--config", str(ar)])
