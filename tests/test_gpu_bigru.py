"""``BiGRU`` (the speech-to-EMA inversion model; reference articulatory/models/pytorch_models.py:22-123) on a MI355X, through the C ABI,
against golden vectors of the REAL reference class (tools/make_golden_bigru.py) and against the CPU restatement tests/bigru_oracle.py.
``pytest -m gpu``.  Values: 2e-5 of max|y|, the project's exact-fp32 bar.
"""

import os

import numpy as np
import pytest
import torch
import yaml

from bigru_oracle import BiGRUOracle
from conftest import E2W_PARAMS, GOLDEN, rel_err, same_across_shapes
from articulatory_amd.bin import decode as D
from articulatory_amd.models import BiGRU, HiFiGANGenerator
from articulatory_amd.utils.synth import synth_bigru_state_dict, synth_state_dict, uniform

pytestmark = pytest.mark.gpu
TOL = 2e-5
CASES = {"full": (400,), "mfcc": (500,), "small": (1, 300)}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "gold_bigru.npz"))


def case_params(g, tag):
    cin, hidden, out, tanh, seed = (int(v) for v in g[tag + "_params"])
    return dict(in_channels=cin, hidden_size=hidden, out_channels=out, use_tanh=bool(tanh)), seed


def build(params, seed):
    assert torch.cuda.is_available()
    sd = synth_bigru_state_dict(params, seed=seed)
    m = BiGRU(**params)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval().to("cuda:0"), sd


_MODELS = {}


def model_of(g, tag):
    """(device model, CPU restatement) of a golden case, built once per module."""
    if tag not in _MODELS:
        params, seed = case_params(g, tag)
        m, sd = build(params, seed)
        _MODELS[tag] = (m, BiGRUOracle(sd, use_tanh=params["use_tanh"]), params, seed)
    return _MODELS[tag]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def test_every_golden_case(gold):
    for tag, frames in CASES.items():
        m, _, params, seed = model_of(gold, tag)
        for T in frames:
            key = f"{tag}_T{T}_x"
            x = gold[key] if key in gold else uniform(seed, f"x.{T}", (1, params["in_channels"], T), -1.0, 1.0)
            y = m(dev(x))
            assert y.shape == (1, params["out_channels"], T) and y.dtype == torch.float32
            err = rel_err(y.cpu().numpy(), gold[f"{tag}_T{T}_y"])
            print(f"{tag}_T{T}: {err:.3g}")
            assert err < TOL, (tag, T)
    assert "libhificar.so" in open("/proc/self/maps").read()


@pytest.mark.parametrize("B", [1, 3])
def test_full_size_model_T2000_vs_restatement(gold, B):
    m, o, params, seed = model_of(gold, "full")
    x = uniform(seed, f"x2000.{B}", (B, params["in_channels"], 2000), -1.0, 1.0)
    err = rel_err(m(dev(x)).cpu().numpy(), o.forward(x).numpy())
    print(f"B={B} T=2000: {err:.3g}")
    assert err < TOL


@pytest.mark.parametrize("tag,B,T", [("full", 1, 1), ("full", 2, 2), ("full", 1, 17), ("small", 3, 2), ("small", 1, 17), ("full", 64, 200),
                                     ("mfcc", 130, 40), ("small", 130, 33)])
def test_edge_sizes(gold, tag, B, T):
    """Single frames, a few frames, and batches on both sides of the point where a workgroup starts sweeping two sequences (2 B > CUs)."""
    m, o, params, seed = model_of(gold, tag)
    x = uniform(seed, f"edge.{B}.{T}", (B, params["in_channels"], T), -1.0, 1.0)
    err = rel_err(m(dev(x)).cpu().numpy(), o.forward(x).numpy())
    print(f"{tag} B={B} T={T}: {err:.3g}")
    assert err < TOL


@pytest.mark.parametrize("tag", ["small", "full"])
def test_ragged_batch_equals_alone(gold, tag):
    m, o, params, seed = model_of(gold, tag)
    lens = [300, 1, 137, 300]
    x = gold["small_ragged_x"] if tag == "small" else uniform(seed, "ragged", (4, params["in_channels"], 300), -1.0, 1.0)
    xd = dev(x)
    y = m(xd, lengths=lens)
    assert y.shape == (4, params["out_channels"], 300)
    for b, n in enumerate(lens):
        alone = m(xd[b:b + 1, :, :n].contiguous())
        assert same_across_shapes(alone[0], y[b, :, :n]), (b, n)
        assert not y[b, :, n:].any(), b
    ref = gold["small_ragged_y"] if tag == "small" else o.forward(x, lengths=lens).numpy()
    assert rel_err(y.cpu().numpy(), ref) < TOL
    # lengths as a device tensor, and a zero-length row
    y2 = m(xd, lengths=torch.tensor([300, 0, 137, 300], device="cuda:0"))
    assert torch.equal(y2[[0, 2, 3]], y[[0, 2, 3]]) and not y2[1].any()
    with pytest.raises(RuntimeError, match="lengths"):
        m(xd, lengths=[300, 1, 137, 301])


def test_repeatable_and_workspace_regrows(gold):
    _, o, params, seed = model_of(gold, "mfcc")
    m, _ = build(params, seed)  # a model of its own: its workspace has seen no other shape
    x = dev(uniform(seed, "rep", (2, params["in_channels"], 64), -1.0, 1.0))
    y1 = m(x)
    y2 = m(x)
    assert torch.equal(y1, y2)
    small_ws = m._workspace_buf.numel()
    xl = uniform(seed, "rep.long", (2, params["in_channels"], 3000), -1.0, 1.0)
    yl = m(dev(xl))
    assert m._workspace_buf.numel() > small_ws
    assert rel_err(yl.cpu().numpy(), o.forward(xl).numpy()) < TOL
    assert torch.equal(m(x), y1)  # and the short shape again, in the larger buffer


def test_non_default_stream(gold):
    m, _, params, seed = model_of(gold, "small")
    x = dev(gold["small_T300_x"])
    want = m(x)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = m(x)
    s.synchronize()
    assert torch.equal(got, want)
    assert rel_err(got.cpu().numpy(), gold["small_T300_y"]) < TOL


def test_inference_with_and_without_normalisation(gold, tmp_path):
    params, seed = case_params(gold, "small")
    m, _ = build(params, seed)
    np.save(tmp_path / "stats.npy", gold["small_stats"])
    m.register_stats(str(tmp_path / "stats.npy"))
    m = m.to("cuda:0")
    c = gold["small_inf_c"]
    y = m.inference(c)  # ndarray in, normalize_before=True by default (pytorch_models.py:86)
    assert y.shape == (200, 12) and rel_err(y.cpu().numpy(), gold["small_inf_y"]) < TOL
    y = m.inference(dev(c), normalize_before=False)
    assert rel_err(y.cpu().numpy(), gold["small_inf_raw_y"]) < TOL
    y3 = m.inference(dev(c).t().unsqueeze(0), normalize_before=False)  # a 3-D (1, C, T) tensor is taken apart first (:97-99)
    assert torch.equal(y3, y)
    # mask / spk_id / ph / ar / spk are accepted and ignored, as in the reference
    x = dev(gold["small_T300_x"])
    assert torch.equal(m(x, mask=torch.ones(1), spk_id=torch.zeros(1), spk=torch.zeros(1, 3), ar=torch.zeros(1), ph=torch.zeros(1)), m(x))


def test_decode_art_mode_end_to_end(gold, tmp_path):
    """articulatory-decode in ``art`` mode on the device: checkpoint + config.yml + stats.npy in, <utt>_gen.npy (T, out_channels) out; the
    files written at --batch-size 1 (model.inference per utterance) and --batch-size 4 (ragged batches) are equal."""
    params, seed = case_params(gold, "small")
    sd = synth_bigru_state_dict(params, seed=seed)
    torch.save({"model": {"generator": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}}, tmp_path / "checkpoint-1steps.pkl")
    (tmp_path / "config.yml").write_text(yaml.safe_dump(dict(generator_type="BiGRU", generator_params=params, dataset_mode="art", format="npy")))
    np.save(tmp_path / "stats.npy", gold["small_stats"])
    dump = tmp_path / "dump"
    dump.mkdir()
    c = gold["small_inf_c"]
    feats = {"uttA": c, "uttB": c[:77].copy(), "uttC": c[40:41].copy(), "uttD": c[10:150].copy(), "uttE": c[::-1].copy()}
    for u, f in feats.items():
        np.save(dump / f"{u}-feats.npy", f)
    for bs in (1, 4):
        D.main(["--dumpdir", str(dump), "--outdir", str(tmp_path / f"out{bs}"), "--checkpoint", str(tmp_path / "checkpoint-1steps.pkl"),
                "--normalize-before", "--batch-size", str(bs), "--verbose", "0"])
    y = np.load(tmp_path / "out1" / "uttA_gen.npy")
    assert y.shape == (200, 12) and y.dtype == np.float32 and rel_err(y, gold["small_inf_y"]) < TOL
    for u, f in feats.items():
        a, b = np.load(tmp_path / "out1" / f"{u}_gen.npy"), np.load(tmp_path / "out4" / f"{u}_gen.npy")
        assert a.shape == (len(f), 12) and np.array_equal(a, b), u


def test_features_to_ema_to_speech_stays_on_the_device(gold):
    """A BiGRU with out_channels = 13 (pitch first, then the 12 EMA dimensions) feeds HiFiGANGenerator.ar_synthesis directly; the waveform
    is bit-identical to the same two steps with a host round trip in between."""
    inv_params = dict(in_channels=80, hidden_size=64, out_channels=13, use_tanh=False)
    inv, _ = build(inv_params, 5110)
    gen_params = dict(E2W_PARAMS, channels=64)
    gen = HiFiGANGenerator(**gen_params)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(gen_params, seed=1234).items()})
    gen.remove_weight_norm()
    gen = gen.eval().to("cuda:0")
    x = dev(uniform(5110, "chain.x", (2, 80, 60), -1.0, 1.0))
    with torch.no_grad():
        ema = inv(x)
        assert ema.is_cuda and ema.shape == (2, 13, 60)
        wav = gen.ar_synthesis(ema, 25)
        ema_host = ema.cpu().numpy()
        wav_rt = gen.ar_synthesis(torch.from_numpy(ema_host).to("cuda:0"), 25)
    assert wav.shape == (2, 60 * gen.hop) and torch.isfinite(wav).all() and wav.abs().max() > 0
    assert torch.equal(wav, wav_rt)
