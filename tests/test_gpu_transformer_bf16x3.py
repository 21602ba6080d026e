"""``Transformer(precision="bf16x3")`` on a MI355X: every GEMM of the eval-mode forward in the conv engine's bf16x3 kernels, everything else
fp32.  ``pytest -m gpu``.  Results are compared against the golden vectors of the REAL reference class and against the float64 restatement
tests/transformer_oracle.py — never against the CPU emulation (tests/transformer_bf16x3_emulation.py), which only set the bar: its error
on these very inputs is at most 1.8e-5 of max|y|, below 1e-4, so the bar is the project's bf16x3 bar, 2e-4 of max|y|.
"""

import copy
import ctypes
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN, rel_err
from transformer_bf16x3_emulation import HEAD_CASES, WIDTH_CASES
from transformer_oracle import TransformerOracle
from articulatory_amd import _native
from articulatory_amd.bin import decode as D
from articulatory_amd.models import Transformer
from articulatory_amd.utils.synth import synth_transformer_state_dict, uniform

pytestmark = pytest.mark.gpu
TOL = 2e-4
TAPS = ("w_raw_in", "layers.0.norm1", "layers.0", "layers.1")


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLDEN, "gold_transformer.npz")))
    g.update(np.load(os.path.join(GOLDEN, "gold_transformer_taps.npz")))
    return g


def case_params(g, tag):
    cin, cout, elayers, hidden, seed = (int(v) for v in g[tag + "_params"])
    return dict(in_channels=cin, out_channels=cout, elayers=elayers, hidden_dim=hidden), seed


def build(params, seed, precision="bf16x3"):
    assert torch.cuda.is_available()
    sd = synth_transformer_state_dict(params, seed=seed)
    m = Transformer(**params, precision=precision)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval().to("cuda:0"), sd


_MODELS = {}


def small(g, precision="bf16x3"):
    """(device model, constructor keywords, seed) of the small golden case in one arithmetic, built once per module."""
    if precision not in _MODELS:
        params, seed = case_params(g, "small")
        _MODELS[precision] = (build(params, seed, precision)[0], params, seed)
    return _MODELS[precision]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def check(what, got, want):
    err = rel_err(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, want)
    print(f"{what}: {err:.3g}")
    assert err < TOL, what
    return err


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


def test_conv_blocks_tap_is_refused(gold):
    m, params, _ = small(gold)
    buf = torch.zeros((1, 4, params["hidden_dim"]), dtype=torch.float32, device="cuda:0")
    with pytest.raises(ValueError, match="conv_blocks"):
        m.debug_tap("conv_blocks", buf)
    assert m._lib.hificar_xfmr_debug_tap(m._native_handle(), b"conv_blocks", buf.data_ptr(), buf.numel()) == -1  # HIFICAR_E_INVALID


def test_default_size_golden(gold):
    params, seed = case_params(gold, "default")
    m, _ = build(params, seed)
    x = uniform(seed, "x.400", (1, params["in_channels"], 400), -1.0, 1.0)
    check("default_T400", m(dev(x)), gold["default_T400_y"])


def kernel_names(m, x):
    """(result, the kernel names of one profiled forward)"""
    eng = m.engine()
    _native.check(m._lib.hificar_profile_begin(eng), "hificar_profile_begin")
    y = m(x)
    return y, [r["name"] for r in _native.profile_rows(m._lib, eng, 128)[0]]


def test_the_arithmetic_really_ran(gold):
    """By the profile's kernel names: a bf16x3 forward has no exact-fp32 GEMM and an exact-fp32 forward no bf16x3 one; the small kernels'
    bf16x3 variants carry their own names.  The two results differ, by less than the bar."""
    mb, params, seed = small(gold)
    mf, _, _ = small(gold, "f32")
    x = dev(uniform(seed, "x.260", (1, params["in_channels"], 260), -1.0, 1.0))
    yb, tb = kernel_names(mb, x)
    yf, tf = kernel_names(mf, x)
    print(tb)
    print(tf)
    gb, gf = [k for k in tb if k.startswith("conv_")], [k for k in tf if k.startswith("conv_")]
    assert gb and all(k.startswith(("conv_bf16x3_kernel<", "conv_bf16x3nb_kernel<")) for k in gb), gb
    assert gf and all(k.startswith("conv_f32do_kernel<") for k in gf), gf
    assert set(tb) - set(gb) == {"xfmr_rows_split_kernel", "xfmr_ln_kernel<split>", "xfmr_attn_kernel<split>", "xfmr_out_kernel"}, tb
    assert set(tf) - set(gf) == {"xfmr_rows_kernel", "xfmr_ln_kernel", "xfmr_attn_kernel", "xfmr_out_kernel"}, tf
    assert not torch.equal(yb, yf)
    check("bf16x3 against f32", yb, yf.cpu().numpy())
    check("f32 against golden (2e-5)", yf, gold["small_T260_y"])


@pytest.mark.parametrize("case", HEAD_CASES + WIDTH_CASES, ids=lambda c: c[0])
def test_head_sizes_and_width_edges(case):
    """Head sizes 32, 80 and 128 at T = 201 (with the golden cases' 16 and 96: five of the attention's eight split stores, the smallest and the
    largest among them); in_channels == hidden_dim (no residual_path: the input is operand and fp32 residual), in_channels = 5 (padded to
    32), out_channels = 33, T = 65 (one row past a 64-query tile)."""
    tag, params, seed, name, T = case
    m, sd = build(params, seed)
    x = uniform(seed, name, (1, params["in_channels"], T), -1.0, 1.0)
    check(tag, m(dev(x)), TransformerOracle(sd).forward(x).numpy())


def test_ragged_batch(gold):
    m, params, seed = small(gold)
    lens = [int(v) for v in gold["small_ragged_lengths"]]
    x = uniform(seed, "ragged.x", (len(lens), params["in_channels"], max(lens)), -1.0, 1.0)
    xd = dev(x)
    y = m(xd, lengths=lens)
    check("ragged against golden", y, gold["small_ragged_y"])
    for b, n in enumerate(lens):
        alone = m(xd[b:b + 1, :, :n].contiguous())
        assert torch.equal(alone[0], y[b, :, :n]), (b, n)
        assert not y[b, :, n:].any(), b
    xn = xd.clone()
    for b, n in enumerate(lens):
        xn[b, :, n:] = float("nan")  # what the input holds past a length is never used
    assert torch.equal(m(xn, lengths=lens), y)
    keep = [b for b in range(len(lens)) if b != 1]
    y2 = m(xd, lengths=[0 if b == 1 else n for b, n in enumerate(lens)])  # a zero-length row
    assert torch.equal(y2[keep], y[keep]) and not y2[1].any()


def test_workspace_contents_do_not_matter(gold):
    """A (3, 263) forward and then a (1, 70) forward on one handle through the C entry point, the workspace once zero-filled and once
    filled with 0xFF bytes: bitwise the same results."""
    params, seed = case_params(gold, "small")
    m, _ = build(params, seed)
    handle, lib = m._native_handle(), m._lib
    big = dev(uniform(seed, "ws.big", (3, params["in_channels"], 263), -1.0, 1.0))
    one = dev(uniform(seed, "ws.small", (1, params["in_channels"], 70), -1.0, 1.0))
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
            out = torch.empty((B, params["out_channels"], T), dtype=torch.float32, device="cuda:0")
            _native.check(lib.hificar_xfmr_forward(handle, x.data_ptr(), None, None, out.data_ptr(), B, T, ws.data_ptr() + off, n, stream), "forward")
            outs.append(out)
        torch.cuda.synchronize()
        got.append(outs)
    for a, b in zip(*got):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert torch.equal(got[0][0], m(big)) and torch.equal(got[0][1], m(one))


def test_bf16x3_handle_refuses_training_entry_points(gold):
    m, _, _ = small(gold)
    lib, handle = m._lib, m._native_handle()
    assert lib.hificar_xfmr_set_precision(handle, _native.PREC_F32) == -2  # HIFICAR_E_STATE: after finalize
    assert lib.hificar_xfmr_grad_count(handle) == -1
    assert lib.hificar_xfmr_train_workspace_bytes(handle, 2, 64) == 0
    assert b"bf16x3" in lib.hificar_last_error()


def test_switch_after_an_fp32_training_step(gold):
    """One fp32 training step (fused Adam), then set_precision("bf16x3"): the eval result is that of a fresh bf16x3 model loaded from the
    trained state_dict, bitwise; back in f32 the fp32 eval result is reproduced bitwise."""
    params, seed = case_params(gold, "small")
    m, _ = build(params, seed, "f32")
    x = dev(uniform(seed, "train.x", (2, params["in_channels"], 64), -1.0, 1.0))
    m.train()
    m.set_dropout_seed(11)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, fused=True)
    m(x).square().mean().backward()
    opt.step()
    m.eval()
    y32 = m(x)
    m.set_precision("bf16x3")
    y = m(x)
    fresh = Transformer(**params, precision="bf16x3")
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.eval().to("cuda:0")
    assert fresh.precision == "bf16x3"
    assert torch.equal(fresh(x), y)
    assert not torch.equal(y, y32)
    check("trained weights, bf16x3 against f32", y, y32.cpu().numpy())
    with pytest.raises(RuntimeError, match="exact-fp32"):
        m.train()(x)
    m.eval()
    m.set_precision("f32")
    assert torch.equal(m(x), y32)
    assert copy.deepcopy(fresh).precision == "bf16x3"


def test_decode_precision_flag(gold, tmp_path):
    """articulatory-decode --precision bf16x3 in a2m mode: the file is within the bar of the golden inference case; without the flag the file
    is the exact-fp32 model's own result, bit for bit."""
    params, seed = case_params(gold, "small")
    sd = synth_transformer_state_dict(params, seed=seed)
    torch.save({"model": {"generator": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}}, tmp_path / "checkpoint-1steps.pkl")
    (tmp_path / "config.yml").write_text(yaml.safe_dump(dict(generator_type="Transformer", generator_params=params, dataset_mode="a2m", format="npy")))
    dump = tmp_path / "dump"
    dump.mkdir()
    c = uniform(seed, "inference.c", (200, params["in_channels"]), -2.0, 2.0)
    np.save(dump / "uttA-feats.npy", c)
    common = ["--dumpdir", str(dump), "--checkpoint", str(tmp_path / "checkpoint-1steps.pkl"), "--batch-size", "1", "--verbose", "0"]
    D.main(common + ["--outdir", str(tmp_path / "out_default")])
    D.main(common + ["--outdir", str(tmp_path / "out_f32"), "--precision", "f32"])
    D.main(common + ["--outdir", str(tmp_path / "out_x3"), "--precision", "bf16x3"])
    y0, y1, y3 = (np.load(tmp_path / d / "uttA_gen.npy") for d in ("out_default", "out_f32", "out_x3"))
    mf, _, _ = small(gold, "f32")
    assert np.array_equal(y0, mf.inference(dev(c)).cpu().numpy()) and np.array_equal(y0, y1)
    assert rel_err(y0, gold["small_inf_y"]) < 2e-5
    assert y3.shape == y0.shape and not np.array_equal(y3, y0)
    check("decode --precision bf16x3", y3, gold["small_inf_y"])
