"""``Transformer`` (the feature-to-feature encoder; reference articulatory/models/transformer.py:21-105) on a MI355X, through the C ABI,
against golden vectors of the REAL reference class (tools/make_golden_transformer.py) and against the float64 restatement
tests/transformer_oracle.py.  ``pytest -m gpu``.  Values: 2e-5 of max|y|, the project's exact-fp32 bar.
"""

import ctypes
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN, rel_err
from transformer_oracle import EDGE_FRAMES, TransformerOracle
from articulatory_amd import _native
from articulatory_amd.bin import decode as D
from articulatory_amd.models import Transformer
from articulatory_amd.utils.synth import synth_transformer_state_dict, uniform

pytestmark = pytest.mark.gpu
TOL = 2e-5
CASES = {"default": (400,), "small": (1, 100, 101, 260)}
TAPS = ("conv_blocks", "w_raw_in", "layers.0.norm1", "layers.0", "layers.1.norm1", "layers.1")


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLDEN, "gold_transformer.npz")))
    g.update(np.load(os.path.join(GOLDEN, "gold_transformer_taps.npz")))
    return g


def case_params(g, tag):
    cin, cout, elayers, hidden, seed = (int(v) for v in g[tag + "_params"])
    return dict(in_channels=cin, out_channels=cout, elayers=elayers, hidden_dim=hidden), seed


def build(params, seed):
    assert torch.cuda.is_available()
    sd = synth_transformer_state_dict(params, seed=seed)
    m = Transformer(**params)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval().to("cuda:0"), sd


_MODELS = {}


def model_of(g, tag):
    """(device model, float64 restatement) of a golden case, built once per module."""
    if tag not in _MODELS:
        params, seed = case_params(g, tag)
        m, sd = build(params, seed)
        _MODELS[tag] = (m, TransformerOracle(sd), params, seed)
    return _MODELS[tag]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def test_every_golden_case_and_tap(gold):
    for tag, frames in CASES.items():
        m, _, params, seed = model_of(gold, tag)
        for T in frames:
            x = uniform(seed, f"x.{T}", (1, params["in_channels"], T), -1.0, 1.0)
            bufs = {}
            if tag == "small":
                for name in TAPS:
                    bufs[name] = torch.zeros((1, T, params["hidden_dim"]), dtype=torch.float32, device="cuda:0")
                    m.debug_tap(name, bufs[name])
            y = m(dev(x))
            m.debug_tap(None)
            assert y.shape == (1, params["out_channels"], T) and y.dtype == torch.float32
            err = rel_err(y.cpu().numpy(), gold[f"{tag}_T{T}_y"])
            print(f"{tag}_T{T}: {err:.3g}")
            assert err < TOL, (tag, T)
            for name, buf in bufs.items():
                e = rel_err(buf.cpu().numpy(), gold[f"{tag}_T{T}_tap_{name}"])
                print(f"{tag}_T{T} tap {name}: {e:.3g}")
                assert e < TOL, (tag, T, name)
    assert "libhificar.so" in open("/proc/self/maps").read()


@pytest.mark.parametrize("T", EDGE_FRAMES)
def test_attention_edges(gold, T):
    """The band edge (|k - q| = 99 against 100) and the tile and key-block edges of a 32- or 64-row tiling."""
    m, o, params, seed = model_of(gold, "small")
    x = uniform(seed, f"edge.{T}", (1, params["in_channels"], T), -1.0, 1.0)
    err = rel_err(m(dev(x)).cpu().numpy(), o.forward(x).numpy())
    print(f"T={T}: {err:.3g}")
    assert err < TOL


def test_batch_of_three_T263(gold):
    m, o, params, seed = model_of(gold, "small")
    x = uniform(seed, "edge.b3", (3, params["in_channels"], 263), -1.0, 1.0)
    err = rel_err(m(dev(x)).cpu().numpy(), o.forward(x).numpy())
    print(f"B=3 T=263: {err:.3g}")
    assert err < TOL


@pytest.mark.parametrize("hidden", [256, 384, 512, 640, 896])
def test_other_head_sizes(hidden):
    """Head sizes 32 to 112: with the golden cases' 16 and 96 every xfmr_attn_kernel<D, false> instantiation but 128."""
    params = dict(in_channels=24, out_channels=40, elayers=1, hidden_dim=hidden)
    m, sd = build(params, 6200 + hidden)
    x = uniform(6200 + hidden, "x.201", (1, 24, 201), -1.0, 1.0)
    err = rel_err(m(dev(x)).cpu().numpy(), TransformerOracle(sd).forward(x).numpy())
    print(f"hidden {hidden}: {err:.3g}")
    assert err < TOL


def test_ragged_batch_at_another_head_size():
    """test_ragged_batch_equals_alone_bitwise at head size 80, whose lengths branch no other test takes: a ragged batch is bitwise its
    sequences alone, each of which meets the float64 restatement."""
    hidden, lens = 640, [201, 100]
    params = dict(in_channels=24, out_channels=40, elayers=1, hidden_dim=hidden)
    m, sd = build(params, 6200 + hidden)
    o = TransformerOracle(sd)
    x = uniform(6200 + hidden, "ragged.x", (2, 24, 201), -1.0, 1.0)
    xd = dev(x)
    y = m(xd, lengths=lens)
    assert y.shape == (2, 40, 201)
    for b, n in enumerate(lens):
        alone = m(xd[b:b + 1, :, :n].contiguous())
        assert torch.equal(alone[0], y[b, :, :n]), (b, n)
        assert not y[b, :, n:].any(), b
        err = rel_err(alone.cpu().numpy(), o.forward(x[b:b + 1, :, :n]).numpy())
        print(f"hidden {hidden} ragged, sequence {b} ({n} frames): {err:.3g}")
        assert err < TOL
    xn = xd.clone()
    xn[1, :, 100:] = float("nan")  # what the input holds past a length is never used
    assert torch.equal(m(xn, lengths=lens), y)


def test_default_size_batch(gold):
    m, o, params, seed = model_of(gold, "default")
    x = uniform(seed, "x.b2.330", (2, params["in_channels"], 330), -1.0, 1.0)
    err = rel_err(m(dev(x)).cpu().numpy(), o.forward(x).numpy())
    print(f"default B=2 T=330: {err:.3g}")
    assert err < TOL


def test_ragged_batch_equals_alone_bitwise(gold):
    m, _, params, seed = model_of(gold, "small")
    lens = [int(v) for v in gold["small_ragged_lengths"]]
    x = uniform(seed, "ragged.x", (len(lens), params["in_channels"], max(lens)), -1.0, 1.0)
    xd = dev(x)
    y = m(xd, lengths=lens)
    assert y.shape == (4, params["out_channels"], 260)
    err = rel_err(y.cpu().numpy(), gold["small_ragged_y"])
    print(f"ragged vs golden: {err:.3g}")
    assert err < TOL
    for b, n in enumerate(lens):
        alone = m(xd[b:b + 1, :, :n].contiguous())
        assert torch.equal(alone[0], y[b, :, :n]), (b, n)
        assert not y[b, :, n:].any(), b
    # what the input holds past a length is never used
    xn = xd.clone()
    for b, n in enumerate(lens):
        xn[b, :, n:] = float("nan")
    assert torch.equal(m(xn, lengths=lens), y)
    # lengths as a device tensor, and a zero-length row
    y2 = m(xd, lengths=torch.tensor([260, 0, 137, 260], device="cuda:0"))
    assert torch.equal(y2[[0, 2, 3]], y[[0, 2, 3]]) and not y2[1].any()
    with pytest.raises(RuntimeError, match="lengths"):
        m(xd, lengths=[260, 1, 137, 261])


def test_workspace_contents_do_not_matter(gold):
    """Two forwards of different (B, T) on one handle, the smaller after the larger, through the C entry point, with the workspace once
    zero-filled and once filled with 0xFF bytes (NaN as floats): bitwise the same results."""
    params, seed = case_params(gold, "small")
    m, _ = build(params, seed)
    handle, lib = m._native_handle(), m._lib
    big = dev(uniform(seed, "ws.big", (3, params["in_channels"], 230), -1.0, 1.0))
    small = dev(uniform(seed, "ws.small", (2, params["in_channels"], 70), -1.0, 1.0))
    lens = torch.tensor([70, 33], dtype=torch.int32)
    lens_d = lens.to("cuda:0")
    n = lib.hificar_xfmr_workspace_bytes(handle, 3, 230)
    assert n >= lib.hificar_xfmr_workspace_bytes(handle, 2, 70) > 0
    ws = torch.empty(n + 256, dtype=torch.uint8, device="cuda:0")
    off = (-ws.data_ptr()) % 256
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    got = []
    for fill in (0, 0xFF):
        outs = []
        for x, ld, lh in ((big, None, None), (small, lens_d.data_ptr(), lens.data_ptr())):
            ws.fill_(fill)
            B, _, T = x.shape
            out = torch.empty((B, params["out_channels"], T), dtype=torch.float32, device="cuda:0")
            _native.check(lib.hificar_xfmr_forward(handle, x.data_ptr(), ld, lh, out.data_ptr(), B, T, ws.data_ptr() + off, n, stream), "forward")
            outs.append(out)
        torch.cuda.synchronize()
        got.append(outs)
    for a, b in zip(*got):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert torch.equal(got[0][0], m(big)) and torch.equal(got[0][1], m(small, lengths=lens))


def test_inference_and_ignored_arguments(gold):
    m, _, params, seed = model_of(gold, "small")
    c = uniform(seed, "inference.c", (200, params["in_channels"]), -2.0, 2.0)
    y = m.inference(dev(c))
    assert y.shape == (200, params["out_channels"]) and rel_err(y.cpu().numpy(), gold["small_inf_y"]) < TOL
    assert torch.equal(m.inference(c), y)  # an ndarray goes to the model's device
    with pytest.raises(NotImplementedError, match="never normalises"):
        m.inference(dev(c), normalize_before=True)
    x = dev(c).t().unsqueeze(0).contiguous()
    assert torch.equal(m(x, spk_id=torch.zeros(1), ar=torch.zeros(1), ph=torch.zeros(1)), m(x))


def test_decode_a2m_mode_end_to_end(gold, tmp_path):
    """articulatory-decode in ``a2m`` mode on the device: a synthetic checkpoint + config.yml in, <utt>_gen.npy (T, out_channels) out; the files
    written at --batch-size 1 (model.inference per utterance) and --batch-size 4 (ragged batches) are equal."""
    params, seed = case_params(gold, "small")
    sd = synth_transformer_state_dict(params, seed=seed)
    torch.save({"model": {"generator": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}}, tmp_path / "checkpoint-1steps.pkl")
    (tmp_path / "config.yml").write_text(yaml.safe_dump(dict(generator_type="Transformer", generator_params=params, dataset_mode="a2m", format="npy")))
    dump = tmp_path / "dump"
    dump.mkdir()
    c = uniform(seed, "inference.c", (200, params["in_channels"]), -2.0, 2.0)
    feats = {"uttA": c, "uttB": c[:77].copy(), "uttC": c[40:41].copy(), "uttD": c[10:150].copy(), "uttE": c[::-1].copy()}
    for u, f in feats.items():
        np.save(dump / f"{u}-feats.npy", f)
    for bs in (1, 4):
        D.main(["--dumpdir", str(dump), "--outdir", str(tmp_path / f"out{bs}"), "--checkpoint", str(tmp_path / "checkpoint-1steps.pkl"),
                "--batch-size", str(bs), "--verbose", "0"])
    y = np.load(tmp_path / "out1" / "uttA_gen.npy")
    assert y.shape == (200, params["out_channels"]) and y.dtype == np.float32 and rel_err(y, gold["small_inf_y"]) < TOL
    for u, f in feats.items():
        a, b = np.load(tmp_path / "out1" / f"{u}_gen.npy"), np.load(tmp_path / "out4" / f"{u}_gen.npy")
        assert a.shape == (len(f), params["out_channels"]) and np.array_equal(a, b), u
