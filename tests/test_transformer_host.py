"""The Transformer feature model's host side (reference articulatory/models/transformer.py:21-105): state_dict surface, loading, the
restatement the GPU tests measure against, refusals, the C struct, and the ``a2m`` decode path.  No GPU."""

import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, rel_err
from transformer_oracle import EDGE_FRAMES, TransformerOracle
from articulatory_amd import _native
from articulatory_amd.bin import decode as D
from articulatory_amd.models import Transformer
from articulatory_amd.utils import load_model
from articulatory_amd.utils.synth import synth_transformer_state_dict, transformer_param_spec, uniform

TOL = 2e-5
CASES = {"default": (400,), "small": (1, 100, 101, 260)}
SMALL = dict(in_channels=80, out_channels=18, elayers=2, hidden_dim=128)


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLDEN, "gold_transformer.npz")))
    g.update(np.load(os.path.join(GOLDEN, "gold_transformer_taps.npz")))
    return g


def case_params(g, tag):
    cin, cout, elayers, hidden, seed = (int(v) for v in g[tag + "_params"])
    return dict(in_channels=cin, out_channels=cout, elayers=elayers, hidden_dim=hidden), seed


def torch_sd(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


_ORACLES = {}


def oracles(g, tag):
    """(float64 restatement, float32 restatement, params, seed) of a golden case, built once per module."""
    if tag not in _ORACLES:
        params, seed = case_params(g, tag)
        sd = synth_transformer_state_dict(params, seed=seed)
        _ORACLES[tag] = (TransformerOracle(sd), TransformerOracle(sd, dtype=torch.float32), params, seed)
    return _ORACLES[tag]


def test_state_dict_keys_shapes_and_order(gold):
    params, _ = case_params(gold, "default")
    want = open(os.path.join(GOLDEN, "gold_transformer_keys.txt")).read().split()
    sd = Transformer(**params).state_dict()
    assert list(sd.keys()) == want == list(transformer_param_spec(**params).keys())
    for k, shape in transformer_param_spec(**params).items():
        assert tuple(sd[k].shape) == tuple(shape), k
    assert sd["conv_blocks.0.bn1.num_batches_tracked"].dtype == torch.int64
    assert sd["transformer.layers.5.self_attn.w_q"].shape == (8, 768, 96) and sd["transformer.layers.0.self_attn.w_o"].shape == (8, 96, 768)
    assert sd["transformer.layers.3.self_attn.relative_positional.embeddings"].shape == (8, 199, 96, 1)
    assert "conv_blocks.0.residual_path.weight" in sd and "conv_blocks.1.residual_path.weight" not in sd
    # a model whose input is already hidden_dim wide has no 1 x 1 residual path (pytorch_layers.py:108-112)
    assert not any("residual_path" in k for k in Transformer(in_channels=128, out_channels=4, elayers=1, hidden_dim=128).state_dict())
    # constructor keywords and defaults of the reference (transformer.py:22-24)
    sig = inspect.signature(Transformer.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [
        ("in_channels", 8), ("out_channels", 80), ("elayers", 6), ("hidden_dim", 768), ("dropout", .2), ("extra_art", False), ("use_ar", False),
        ("ar_input", 512), ("ar_hidden", 256), ("ar_output", 128), ("use_tanh", False), ("num_ph", None), ("ph_emb_size", 8), ("layer_type", "default")]
    assert list(inspect.signature(Transformer.forward).parameters)[1:] == ["x", "spk_id", "ar", "ph", "lengths"]
    assert inspect.signature(Transformer.inference).parameters["normalize_before"].default is False
    Transformer(**SMALL, dropout=0.5, use_ar=True, ar_input=3, use_tanh=True)  # accepted and unused, as in the reference


def test_reference_layout_checkpoint_loads_strict(tmp_path):
    params = dict(SMALL, out_channels=80)
    sd = synth_transformer_state_dict(params, seed=7)
    m = Transformer(**params)
    res = m.load_state_dict(torch_sd(sd), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), sd[k]), k
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_state_dict({k: v for k, v in torch_sd(sd).items() if k != "conv_blocks.2.bn2.running_var"}, strict=True)
    # load_model: the out_channels > 1 refusal is for the waveform generators only; stats.npy beside the checkpoint is picked up
    torch.save({"model": {"generator": torch_sd(sd)}}, tmp_path / "checkpoint-1steps.pkl")
    config = dict(generator_type="Transformer", generator_params=params, format="npy")
    stats = np.stack([np.linspace(-1, 1, 80), np.linspace(0.5, 2, 80)]).astype(np.float32)
    np.save(tmp_path / "stats.npy", stats)
    model = load_model(str(tmp_path / "checkpoint-1steps.pkl"), config)
    assert isinstance(model, Transformer) and not hasattr(model, "pqmf")
    assert np.array_equal(model.mean.numpy(), stats[0]) and np.array_equal(model.scale.numpy(), stats[1])
    model.remove_weight_norm()  # exists, changes nothing
    assert list(model.state_dict().keys()) == ["mean", "scale"] + list(sd.keys())
    assert set(model.native_state()) == {k for k in sd if not k.endswith("num_batches_tracked")}


def test_restatement_matches_the_reference_goldens(gold):
    """tests/transformer_oracle.py (float64, banded) against every array of the real reference class — outputs and taps — within 4 x the
    array's recorded fp32-vs-float64 deviation: the golden is the class's fp32 run, so a float64 restatement of the same function is one
    such deviation away from it.  Measured: 1.00 x the recorded deviation for every array (the restatement equals the class's float64 run
    to 1e-15)."""
    for tag, frames in CASES.items():
        o, _, params, seed = oracles(gold, tag)
        for T in frames:
            taps = {}
            y = o.forward(uniform(seed, f"x.{T}", (1, params["in_channels"], T), -1.0, 1.0), taps=taps).numpy()
            err, dev = rel_err(y, gold[f"{tag}_T{T}_y"]), float(gold[f"{tag}_T{T}_f32_dev"])
            print(f"{tag}_T{T}: restatement vs golden {err:.3g}, recorded f32 dev {dev:.3g}")
            assert dev <= 2e-6 and err <= 4 * dev
            if tag == "small":
                assert len(taps) == 6
                for name, v in taps.items():
                    key = f"{tag}_T{T}_tap_{name}"
                    assert float(gold[key + "_f32_dev"]) <= 2e-6 and rel_err(v.numpy(), gold[key]) <= 4 * float(gold[key + "_f32_dev"]), key
    o, _, params, seed = oracles(gold, "small")
    c = uniform(seed, "inference.c", (200, params["in_channels"]), -2.0, 2.0)
    assert rel_err(o.inference(c).numpy(), gold["small_inf_y"]) <= 4 * float(gold["small_inf_f32_dev"])
    lens = [int(v) for v in gold["small_ragged_lengths"]]
    x = uniform(seed, "ragged.x", (len(lens), params["in_channels"], max(lens)), -1.0, 1.0)
    yr = o.forward(x, lengths=lens)
    assert rel_err(yr.numpy(), gold["small_ragged_y"]) <= 4 * float(gold["small_ragged_f32_dev"])
    for b, n in enumerate(lens):
        assert not yr[b, :, n:].any()


def gpu_test_shapes(gold):
    """(tag or params, seed, input name, shape) of every comparison tests/test_gpu_transformer.py makes against the restatement."""
    _, _, params, seed = oracles(gold, "small")
    out = [("small", seed, f"edge.{T}", (1, params["in_channels"], T)) for T in EDGE_FRAMES]
    out.append(("small", seed, "edge.b3", (3, params["in_channels"], 263)))
    for hidden in (256, 512):
        out.append((dict(in_channels=24, out_channels=40, elayers=1, hidden_dim=hidden), 6200 + hidden, "x.201", (1, 24, 201)))
    _, _, params, seed = oracles(gold, "default")
    out.append(("default", seed, "x.b2.330", (2, params["in_channels"], 330)))
    return out


def test_float32_restatement_is_within_half_the_bar_on_every_gpu_test_shape(gold):
    """The device runs fp32; it is measured against the float64 restatement at 2e-5 of max|y|.  That bar is fair for a shape only if fp32
    arithmetic itself stays well inside it there: the restatement's own float32 run must be within HALF the bar of its float64 run."""
    worst = 0.0
    for which, seed, name, shape in gpu_test_shapes(gold):
        if isinstance(which, str):
            o64, o32, _, _ = oracles(gold, which)
        else:
            sd = synth_transformer_state_dict(which, seed=seed)
            o64, o32 = TransformerOracle(sd), TransformerOracle(sd, dtype=torch.float32)
        x = uniform(seed, name, shape, -1.0, 1.0)
        err = rel_err(o32.forward(x).numpy(), o64.forward(x).numpy())
        worst = max(worst, err)
        assert err <= TOL / 2, (which, name, shape, err)
    print(f"worst float32 deviation over the GPU tests' shapes: {worst:.3g}")


@pytest.mark.parametrize("T", [99, 100, 101, 230])
def test_banded_attention_equals_the_dense_masked_form(gold, T):
    """Skipping the keys outside |k - q| <= 99 against the T x T form that lowers them by 1e8: the same function (their weights are exactly 0)."""
    _, _, params, seed = oracles(gold, "small")
    sd = synth_transformer_state_dict(params, seed=seed)
    x = uniform(seed, f"x.{T}", (1, params["in_channels"], T), -1.0, 1.0)
    a, b = TransformerOracle(sd).forward(x), TransformerOracle(sd, dense=True).forward(x)
    assert rel_err(a.numpy(), b.numpy()) <= 1e-13
    # and the chunking of the banded form does not matter
    assert rel_err(TransformerOracle(sd, chunk=37).forward(x).numpy(), a.numpy()) <= 1e-13


def test_refusals():
    with pytest.raises(NotImplementedError, match="extra_art"):
        Transformer(extra_art=True)
    with pytest.raises(NotImplementedError, match="num_ph"):
        Transformer(num_ph=40)
    for hidden in (100, 192, 1152, 64):
        with pytest.raises(ValueError, match="hidden_dim"):
            Transformer(hidden_dim=hidden)
    with pytest.raises(ValueError, match="out_channels"):
        Transformer(out_channels=4096)
    for hidden in (128, 256, 512, 768, 1024):  # what the attention kernel is built for
        _native.check_xfmr_params(dict(in_channels=12, out_channels=80, elayers=6, hidden_dim=hidden))
    m = Transformer(**SMALL)
    x = torch.zeros(1, 80, 5)
    with pytest.raises(NotImplementedError, match=r"train\(\) mode"):
        m(x)
    m.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.inference(np.zeros((5, 80), dtype=np.float32))
    with pytest.raises(NotImplementedError, match="never normalises"):
        m.inference(torch.zeros(5, 80), normalize_before=True)
    from articulatory_amd.bin.train import Trainer
    with pytest.raises(NotImplementedError, match="Transformer"):
        Trainer(dict(generator_type="Transformer"), "cpu")


def test_config_struct_matches_header_and_create_checks():
    assert ctypes.sizeof(_native.HificarXfmrConfig) == 16
    hdr = open(os.path.join(REPO, "include", "hificar.h")).read()
    for name, v in (("IN", _native.XFMR_MAX_IN), ("OUT", _native.XFMR_MAX_OUT), ("HIDDEN", _native.XFMR_MAX_HIDDEN), ("LAYERS", _native.XFMR_MAX_LAYERS)):
        assert f"#define HIFICAR_XFMR_MAX_{name} {v}" in hdr
    lib = _native.load_library()
    h = ctypes.c_void_p()
    cfg = _native.make_xfmr_config(SMALL)
    _native.check(lib.hificar_xfmr_create(ctypes.byref(cfg), ctypes.byref(h)), "hificar_xfmr_create")
    try:
        # input rows (80 -> 96 columns) + three row buffers of 128 + one of 3072 floats per frame, B T rounded up to 256 rows
        assert lib.hificar_xfmr_workspace_bytes(h, 2, 300) == 768 * (96 + 3 * 128 + 3072) * 4
        assert lib.hificar_xfmr_workspace_bytes(h, 0, 300) == 0
        w = np.zeros((18, 128), dtype=np.float32)
        shape = (ctypes.c_int64 * 2)(18, 128)
        assert lib.hificar_xfmr_set_weight(h, b"w_out.weight", w.ctypes.data, shape, 2) == 0
        assert lib.hificar_xfmr_set_weight(h, b"w_out.0.weight", w.ctypes.data, shape, 2) == -1
        assert b"unexpected tensor name" in lib.hificar_last_error()
        assert lib.hificar_xfmr_set_weight(h, b"transformer.layers.2.norm1.weight", w.ctypes.data, (ctypes.c_int64 * 1)(128), 1) == -1
        assert b"unexpected tensor name" in lib.hificar_last_error()  # (two layers)
        shape = (ctypes.c_int64 * 2)(128, 18)
        assert lib.hificar_xfmr_set_weight(h, b"w_out.weight", w.ctypes.data, shape, 2) == -1
        assert b"size mismatch" in lib.hificar_last_error()
        assert lib.hificar_xfmr_finalize(h) == -2 and b"Missing key" in lib.hificar_last_error()
        x = np.zeros(4, dtype=np.float32)
        assert lib.hificar_xfmr_forward(h, x.ctypes.data, None, None, x.ctypes.data, 1, 1, None, 0, None) == -2  # before finalize
    finally:
        lib.hificar_xfmr_destroy(h)
    for hidden in (192, 1152):
        bad = _native.make_xfmr_config(dict(SMALL, hidden_dim=hidden))
        assert lib.hificar_xfmr_create(ctypes.byref(bad), ctypes.byref(h)) == -1 and b"hidden_dim" in lib.hificar_last_error()


class _StubModel:
    """Stands in for the device model in the decode loop: (T, C) -> (T, out) by the restatement."""

    def __init__(self, oracle):
        self.o = oracle
        self.calls = []

    def inference(self, c, normalize_before=False):
        self.calls.append(("inference", tuple(c.shape), normalize_before))
        return self.o.inference(c, normalize_before=normalize_before).float()

    def __call__(self, x, lengths=None):
        self.calls.append(("forward", tuple(x.shape), list(lengths)))
        return self.o.forward(x, lengths=lengths).float()


def test_decode_a2m_mode_writes_the_same_files_at_batch_size_1_and_4(gold, tmp_path):
    o, _, params, seed = oracles(gold, "small")
    c = uniform(seed, "inference.c", (200, params["in_channels"]), -2.0, 2.0)
    dump = tmp_path / "dump"
    dump.mkdir()
    feats = {"uttA": c, "uttB": c[:77].copy(), "uttC": c[40:41].copy()}
    for u, f in feats.items():
        np.save(dump / f"{u}-feats.npy", f)
    config = dict(generator_type="Transformer", generator_params=params, dataset_mode="a2m")
    out1, out4 = tmp_path / "out1", tmp_path / "out4"
    out1.mkdir()
    out4.mkdir()
    model = _StubModel(o)
    n, sec = D.decode_features(model, D.iter_features(dumpdir=str(dump)), config, "cpu", str(out1), normalize_before=False)
    assert n == 3 and sec > 0 and [k[0] for k in model.calls] == ["inference"] * 3
    y = np.load(out1 / "uttA_gen.npy")
    assert y.shape == (200, 18) and y.dtype == np.float32 and rel_err(y, gold["small_inf_y"]) <= 4 * float(gold["small_inf_f32_dev"])
    model = _StubModel(o)
    n, _ = D.decode_features(model, D.iter_features(dumpdir=str(dump)), config, "cpu", str(out4), normalize_before=False, batch_size=4)
    assert n == 3 and model.calls == [("forward", (3, 80, 200), [1, 77, 200])]
    for u, f in feats.items():
        a, b = np.load(out1 / f"{u}_gen.npy"), np.load(out4 / f"{u}_gen.npy")
        assert a.shape == (len(f), 18) and np.array_equal(a, b), u
    # the phoneme modes stay refused
    for mode in ("ph2m", "ph2a"):
        import yaml
        bad = tmp_path / f"{mode}.yml"
        bad.write_text(yaml.safe_dump(dict(generator_type="Transformer", generator_params=params, dataset_mode=mode, format="npy")))
        with pytest.raises(NotImplementedError, match=mode):
            D.main(["--dumpdir", str(dump), "--outdir", str(tmp_path / "o"), "--checkpoint", str(tmp_path / "none.pkl"), "--dry-run", "--config", str(bad)])
