"""``Transformer(precision="bf16x3a")`` on a MI355X: the bf16x3 forward with the attention's three products on bf16 MFMAs too
(xfmr_attn16_kernel).  ``pytest -m gpu``.  Results are compared against the golden vectors of the REAL reference class and against the
float64 restatement tests/transformer_oracle.py — never against the CPU emulation (tests/transformer_bf16x3a_emulation.py), which only set
the bar: its error on these very inputs is at most 2e-5 of max|y|, below 1e-4, so the bar is the project's bf16x3 bar,
2e-4 of max|y|.
"""

import ctypes

import numpy as np
import pytest
import torch
import yaml

from conftest import rel_err
from test_gpu_transformer_bf16x3 import TAPS, TOL, build, case_params, check, dev, gold, kernel_names  # noqa: F401 (gold: a fixture)
from transformer_bf16x3a_emulation import ALL_HEAD_CASES, PEAKED_GAIN, peaked_state_dict
from transformer_oracle import EDGE_FRAMES, TransformerOracle
from articulatory_amd import _native
from articulatory_amd.bin import decode as D
from articulatory_amd.models import Transformer
from articulatory_amd.utils.synth import synth_transformer_state_dict, uniform

pytestmark = pytest.mark.gpu
A = "bf16x3a"
_MODELS = {}


def small(g, precision=A):
    """(device model, constructor keywords, seed) of the small golden case in one arithmetic, built once per module."""
    if precision not in _MODELS:
        params, seed = case_params(g, "small")
        _MODELS[precision] = (build(params, seed, precision)[0], params, seed)
    return _MODELS[precision]


@pytest.mark.parametrize("T", [1, 100, 101, 260])
def test_small_golden_cases_and_taps(gold, T):
    m, params, seed = small(gold)
    x = uniform(seed, f"x.{T}", (1, params["in_channels"], T), -1.0, 1.0)
    bufs = {}
    if T == 260:
        for name in TAPS:
            bufs[name] = torch.zeros((1, T, params["hidden_dim"]), dtype=torch.float32, device="cuda:0")
            m.debug_tap(name, bufs[name])
    try:
        y = m(dev(x))
    finally:
        m.debug_tap(None)
    assert y.shape == (1, params["out_channels"], T) and y.dtype == torch.float32
    check(f"small_T{T}", y, gold[f"small_T{T}_y"])
    for name, buf in bufs.items():
        check(f"small_T{T} tap {name}", buf, gold[f"small_T{T}_tap_{name}"])


def test_default_size_golden(gold):
    params, seed = case_params(gold, "default")
    m, _ = build(params, seed, A)
    x = uniform(seed, "x.400", (1, params["in_channels"], 400), -1.0, 1.0)
    check("default_T400", m(dev(x)), gold["default_T400_y"])


@pytest.mark.parametrize("case", ALL_HEAD_CASES, ids=lambda c: c[0])
def test_all_eight_head_sizes(case):
    """Head sizes 16 .. 128 at T = 201; 16, 48, 80 and 112 are no multiple of 32: their key rows are padded with zero channels in LDS."""
    tag, params, seed, name, T = case
    m, sd = build(params, seed, A)
    x = uniform(seed, name, (1, params["in_channels"], T), -1.0, 1.0)
    check(tag, m(dev(x)), TransformerOracle(sd).forward(x).numpy())


@pytest.fixture(scope="module")
def edge_model():
    tag, params, seed, _, _ = ALL_HEAD_CASES[0]  # one layer, hidden 128 (every head size has 64-key blocks: no second model)
    m, sd = build(params, seed, A)
    return m, TransformerOracle(sd), params, seed


@pytest.mark.parametrize("T", EDGE_FRAMES)
def test_edge_lengths(edge_model, T):
    """The band edge (|k - q| = 99 against 100), the 64-query tile edge and the 64-key block edges."""
    m, oracle, params, seed = edge_model
    x = uniform(seed, f"edge.{T}", (1, params["in_channels"], T), -1.0, 1.0)
    check(f"edge T={T}", m(dev(x)), oracle.forward(x).numpy())


def _ragged(m, x, lens, want, what):
    xd = dev(x)
    y = m(xd, lengths=lens)
    check(what, y, want)
    for b, n in enumerate(lens):
        if n:
            alone = m(xd[b:b + 1, :, :n].contiguous())
            assert torch.equal(alone[0], y[b, :, :n]), (b, n)
        assert not y[b, :, n:].any(), b
    xn = xd.clone()
    for b, n in enumerate(lens):
        xn[b, :, n:] = float("nan")  # what the input holds past a length is never used
    assert torch.equal(m(xn, lengths=lens), y)
    return xd, y


def test_ragged_batch(gold):
    m, params, seed = small(gold)
    lens = [int(v) for v in gold["small_ragged_lengths"]]
    x = uniform(seed, "ragged.x", (len(lens), params["in_channels"], max(lens)), -1.0, 1.0)
    sd = synth_transformer_state_dict(params, seed=seed)
    xd, y = _ragged(m, x, lens, gold["small_ragged_y"], "ragged against golden")
    check("ragged against the restatement", y, TransformerOracle(sd).forward(x, lengths=lens).numpy())
    keep = [b for b in range(len(lens)) if b != 1]
    y2 = m(xd, lengths=[0 if b == 1 else n for b, n in enumerate(lens)])  # a zero-length row
    assert torch.equal(y2[keep], y[keep]) and not y2[1].any()
    # lengths at the tile and block edges, a zero-length row among them
    lens = [260, 0, 1, 64, 65, 137]
    x = uniform(seed, "ragged.edges.x", (len(lens), params["in_channels"], max(lens)), -1.0, 1.0)
    _, y = _ragged(m, x, lens, TransformerOracle(sd).forward(x, lengths=lens).numpy(), "ragged edges against the restatement")
    assert not y[1].any()


def test_peaked_softmax(gold):
    """Every self_attn.w_q times 4: logits up to 23 and a mean top probability of 0.48 (the synthetic weights alone give nearly flat softmaxes)."""
    params, seed = case_params(gold, "small")
    sd = peaked_state_dict(synth_transformer_state_dict(params, seed=seed), PEAKED_GAIN)
    m = Transformer(**params, precision=A)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.eval().to("cuda:0")
    x = uniform(seed, "x.260", (1, params["in_channels"], 260), -1.0, 1.0)
    check("w_q gain 4, T=260", m(dev(x)), TransformerOracle(sd).forward(x).numpy())


def test_the_arithmetic_really_ran(gold):
    """By the profile's kernel names: a bf16x3a forward launches xfmr_attn16_kernel and no xfmr_attn_kernel, a bf16x3 forward the reverse,
    and nothing else differs.  The results differ, both within the bar; the bf16x3 model's is bitwise what it was before the bf16x3a ran."""
    mb, params, seed = small(gold, "bf16x3")
    x = dev(uniform(seed, "x.260", (1, params["in_channels"], 260), -1.0, 1.0))
    yb, tb = kernel_names(mb, x)
    ma, _, _ = small(gold)
    ya, ta = kernel_names(ma, x)
    print(ta)
    print(tb)
    assert "xfmr_attn16_kernel" in ta and not any(k.startswith("xfmr_attn_kernel") for k in ta), ta
    assert "xfmr_attn_kernel<split>" in tb and "xfmr_attn16_kernel" not in tb, tb
    assert set(ta) - {"xfmr_attn16_kernel"} == set(tb) - {"xfmr_attn_kernel<split>"}
    assert not torch.equal(ya, yb)
    check("bf16x3a against golden", ya, gold["small_T260_y"])
    check("bf16x3 against golden", yb, gold["small_T260_y"])
    assert torch.equal(mb(x), yb)


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
def test_workspace_contents_do_not_matter(gold, ragged):
    """A (3, 263) forward and then a (1, 70) forward on one handle through the C entry point, the workspace once zero-filled and once
    filled with 0xFF bytes (NaN as fp32 and as bf16): finite and bitwise the same results.  Key rows past a block's end are written as
    zeros in LDS, never copied."""
    m, params, seed = small(gold)
    handle, lib = m._native_handle(), m._lib
    big = dev(uniform(seed, "ws.big", (3, params["in_channels"], 263), -1.0, 1.0))
    one = dev(uniform(seed, "ws.small", (1, params["in_channels"], 70), -1.0, 1.0))
    lens = {3: [263, 5, 130], 1: [33]}
    n = lib.hificar_xfmr_workspace_bytes(handle, 3, 263)
    assert n >= lib.hificar_xfmr_workspace_bytes(handle, 1, 70) > 0
    ws = torch.empty(n + 256, dtype=torch.uint8, device="cuda:0")
    off = (-ws.data_ptr()) % 256
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    got = []
    for fill in (0, 0xFF):
        outs = []
        for x in (big, one):
            ws.fill_(fill)
            B, _, T = x.shape
            ld = torch.tensor(lens[B], dtype=torch.int32, device="cuda:0") if ragged else None
            out = torch.empty((B, params["out_channels"], T), dtype=torch.float32, device="cuda:0")
            _native.check(lib.hificar_xfmr_forward(handle, x.data_ptr(), ld.data_ptr() if ragged else None, None, out.data_ptr(), B, T,
                                                   ws.data_ptr() + off, n, stream), "forward")
            torch.cuda.synchronize()
            outs.append(out)
        got.append(outs)
    for a, b in zip(*got):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    for x, a in zip((big, one), got[0]):
        assert torch.equal(a, m(x, lengths=lens[x.shape[0]]) if ragged else m(x))


def test_two_forwards_are_bitwise_equal(gold):
    m, params, seed = small(gold)
    x = dev(uniform(seed, "det.x", (4, params["in_channels"], 203), -1.0, 1.0))
    assert torch.equal(m(x), m(x))
    assert torch.equal(m(x, lengths=[203, 1, 64, 150]), m(x, lengths=[203, 1, 64, 150]))


def test_switching_arithmetics(gold):
    params, seed = case_params(gold, "small")
    m, _ = build(params, seed, "f32")
    x = dev(uniform(seed, "x.101", (1, params["in_channels"], 101), -1.0, 1.0))
    y32 = m(x)
    m.set_precision(A)
    ya = m(x)
    m.set_precision("bf16x3")
    y3 = m(x)
    m.set_precision("f32")
    assert torch.equal(m(x), y32)
    assert not torch.equal(ya, y32) and not torch.equal(ya, y3)
    check("bf16x3a after the switch", ya, gold["small_T101_y"])
    check("bf16x3 after the switch", y3, gold["small_T101_y"])
    ma, _, _ = small(gold)
    assert torch.equal(ma(x), ya)  # ... what a model built in this arithmetic computes


def test_decode_precision_flag(gold, tmp_path):
    """articulatory-decode --precision bf16x3a in a2m mode: the file is within the bar of --precision f32's, and not equal to it."""
    params, seed = case_params(gold, "small")
    sd = synth_transformer_state_dict(params, seed=seed)
    torch.save({"model": {"generator": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}}, tmp_path / "checkpoint-1steps.pkl")
    (tmp_path / "config.yml").write_text(yaml.safe_dump(dict(generator_type="Transformer", generator_params=params, dataset_mode="a2m", format="npy")))
    dump = tmp_path / "dump"
    dump.mkdir()
    np.save(dump / "uttA-feats.npy", uniform(seed, "inference.c", (200, params["in_channels"]), -2.0, 2.0))
    common = ["--dumpdir", str(dump), "--checkpoint", str(tmp_path / "checkpoint-1steps.pkl"), "--batch-size", "1", "--verbose", "0"]
    D.main(common + ["--outdir", str(tmp_path / "out_f32"), "--precision", "f32"])
    D.main(common + ["--outdir", str(tmp_path / "out_a"), "--precision", A])
    y1, ya = (np.load(tmp_path / d / "uttA_gen.npy") for d in ("out_f32", "out_a"))
    assert ya.shape == y1.shape and not np.array_equal(ya, y1)
    check("decode --precision bf16x3a against --precision f32", ya, y1)
    assert rel_err(ya, gold["small_inf_y"]) < TOL
