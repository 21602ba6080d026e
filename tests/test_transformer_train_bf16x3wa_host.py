"""The Transformer's opt-in bf16x3wa TRAINING arithmetic (bf16x3w, and the training attention's query-tiled kernels on bf16 MFMAs too), as far
as it goes without a device: the CPU emulation that set the GPU tests' bars (tests/transformer_train_bf16x3wa_emulation.py), what it moves
against the bf16x3w emulation, the Python surface, the trainer's config key and the C ABI's refusals."""

import copy
import ctypes
import logging
import os
import pickle

import pytest
import torch

import transformer_ragged_oracle as R
import transformer_train_bf16x3_emulation as E
import transformer_train_bf16x3w_emulation as EW
import transformer_train_bf16x3wa_emulation as EA
import transformer_train_oracle as O
from conftest import E2W_PARAMS, REPO
from test_transformer_train_host import config
from articulatory_amd import _native
from articulatory_amd.bin import train as T
from articulatory_amd.models import Transformer

E_INVALID, E_STATE = -1, -2


# ------------------------------------------------------------------------------------------------ the emulation and its bars
@pytest.fixture(scope="module")
def emulated():
    return EA.emulated_errors(verbose=True)


def test_recorded_bars_follow_the_rule():
    for k, e in EA.EMULATED.items():
        if k == "out":
            want = 2e-4 if e <= 5e-5 else 4 * e
        else:
            want = EW.BARS_X3W[k] if e <= EW.BARS_X3W[k] / 4 else 4 * e
        assert EA.BARS_X3WA[k] == want, k
    assert set(EA.EMULATED) == set(EW.EMULATED) == set(EA.BARS_X3WA)
    assert EA.BARS_X3WA["out"] < E.NORTH_STAR_TOL
    assert all(EA.BARS_X3WA[k] >= EW.BARS_X3W[k] for k in EA.BARS_X3WA)  # never tighter than the arithmetic it extends
    # the cases are the GPU file's, and every head size's instantiation is among them
    assert set(EA.DENSE_CASES + EA.HEAD_CASES) <= set(O.SHAPES) and set(EA.EDGE_CASES) <= set(O.EDGE_SHAPES) and set(EA.RAGGED_CASES) <= set(R.RAGGED_SHAPES)
    shapes = dict(O.SHAPES, **O.EDGE_SHAPES)
    assert {shapes[n][0]["hidden_dim"] // 8 for n in EA.ALL_DENSE} == {16, 32, 48, 64, 80, 96, 112, 128}


def test_emulated_errors_are_below_a_quarter_of_the_bars(emulated):
    worst, gap = emulated
    assert set(worst) == set(EA.BARS_X3WA)
    for k, e in sorted(worst.items()):
        print(f"  {k}: emulated {e:.3g}, recorded {EA.EMULATED[k]:g}, device bar {EA.BARS_X3WA[k]:g}")
        assert 0 < e <= EA.EMULATED[k] and e <= EA.BARS_X3WA[k] / 4, k
    assert gap < E.X3_OUT_BAR


def test_the_emulation_reroutes_the_attention_and_nothing_upstream_of_it():
    """Against the bf16x3w emulation on t65: the conv_blocks batch statistics lie upstream of the first attention and are equal to the bit;
    out and every gradient that the attention reaches move, and stay within a quarter of the bars of float64."""
    name = "t65"
    with EW.emulating():
        a = O.restatement(name, torch.float64)
    with EA.emulating():
        b = O.restatement(name, torch.float64)
    assert O.banded_attention_train is EA._attention and O.F is torch.nn.functional and E.linear3 is EW._linear3  # (the reroutes are undone)
    assert torch.equal(a["stats"], b["stats"]) and all(torch.equal(a["running"][k], v) for k, v in b["running"].items())
    assert not torch.equal(a["out"], b["out"]) and not torch.equal(a["dx"], b["dx"])
    # every gradient that depends on the attention at all: with an L1 loss, those of w_out.bias and of the last norm2's bias are sums of
    # sign(y - t) (through w_out) over the rows, whatever the layers below computed
    fixed = {"w_out.bias", f"transformer.layers.{O.BASE['elayers'] - 1}.norm2.bias"}
    assert set(a["grads"]) == set(b["grads"]) and {k for k, g in b["grads"].items() if torch.equal(a["grads"][k], g)} == fixed
    ref = O.restatement(name, torch.float64, gates=b["sides"])
    for k, (e, bar) in EA.errors_x3wa(b, ref).items():
        assert e <= bar / 4, (k, e, bar)


def test_the_rerouted_attention_is_the_restatement_when_nothing_is_split(monkeypatch):
    """The hand-written backward itself: with the split products replaced by exact ones, out and all four gradients are autograd's of
    banded_attention_train, with and without a dropout mask, over more than one query chunk."""
    monkeypatch.setattr(EA, "einsum3", lambda eq, a, b: torch.einsum(eq, a, b))
    g = torch.Generator().manual_seed(5)
    B, H, T, d = 2, 2, 150, 8
    mask = (torch.rand((B, H, T, T), generator=g, dtype=torch.float64) > 0.3).double() / 0.7
    for m in (None, mask):
        leaves = [torch.randn(s, generator=g, dtype=torch.float64, requires_grad=True) for s in ((B, H, T, d),) * 3 + ((H, 199, d),)]
        w = torch.randn((B, H, T, d), generator=g, dtype=torch.float64)
        want = O.banded_attention_train(*leaves, m, chunk=64)
        gw = torch.autograd.grad((want * w).sum(), leaves)
        got = EA.attention3(*leaves, m, chunk=64)
        gg = torch.autograd.grad((got * w).sum(), leaves)
        assert float((got - want).detach().abs().max()) < 1e-12
        for x, y in zip(gg, gw):
            assert float((x - y).abs().max()) < 1e-12 * max(1.0, float(y.abs().max()))


# ------------------------------------------------------------------------------------------------ the Python surface and the C ABI
def test_keyword_setter_copies_and_refusals():
    assert _native.PREC_BF16X3WA == 4 and _native.XFMR_TRAIN_PRECISIONS == dict(_native.TRAIN_PRECISIONS, bf16x3wa=4)
    assert _native.TRAIN_PRECISIONS == {"f32": 0, "bf16x3": 1, "bf16x3w": 2} and "bf16x3wa" not in _native.XFMR_PRECISIONS
    m = Transformer(train_precision="bf16x3wa", **O.BASE)
    assert m.train_precision == "bf16x3wa" and m.precision == "f32"
    assert copy.deepcopy(m).train_precision == "bf16x3wa" and pickle.loads(pickle.dumps(m)).train_precision == "bf16x3wa"
    assert not any("precision" in k for k in m.state_dict())
    for to in ("bf16x3w", "bf16x3", "f32", "bf16x3wa"):  # (no handle yet: the choice alone)
        m.set_train_precision(to)
        assert m.train_precision == to
    # the inference arithmetic does not know the value
    with pytest.raises(ValueError, match="precision must be one of"):
        Transformer(precision="bf16x3wa", **O.BASE)
    with pytest.raises(ValueError, match="precision must be one of"):
        Transformer(**O.BASE).set_precision("bf16x3wa")
    for inference in ("bf16x3", "bf16x3a"):
        with pytest.raises(ValueError, match="inference-only"):
            Transformer(precision=inference, train_precision="bf16x3wa", **O.BASE)
        with pytest.raises(ValueError, match="inference-only"):
            Transformer(precision=inference, **O.BASE).set_train_precision("bf16x3wa")
        with pytest.raises(ValueError, match="inference-only"):
            m.set_precision(inference)
    for bad in ("bf16x3WA", "bf16x3aw", 4):
        with pytest.raises(ValueError, match="train_precision must be one of"):
            Transformer(train_precision=bad, **O.BASE)
        with pytest.raises(ValueError, match="train_precision must be one of"):
            Transformer(**O.BASE).set_train_precision(bad)
    with pytest.raises(NotImplementedError, match="on the device only"):
        Transformer(train_precision="bf16x3wa", **O.BASE).train()(torch.zeros(2, 12, 5))


def test_the_trainer_reads_the_config_key(caplog):
    cpu = torch.device("cpu")
    with caplog.at_level(logging.INFO):
        tr = T.InversionTrainer(config(train_precision="bf16x3wa"), cpu)
    assert tr.G.train_precision == "bf16x3wa" and tr.G.precision == "f32" and tr.train_precision == "bf16x3wa"
    assert "training arithmetic bf16x3wa" in caplog.records[0].getMessage()
    bigru = dict(config(), generator_type="BiGRU", generator_params=dict(in_channels=12, out_channels=8))
    with pytest.raises(NotImplementedError, match="train_precision bf16x3wa is built for generator_type Transformer"):
        T.InversionTrainer(dict(bigru, train_precision="bf16x3wa"), cpu)
    with pytest.raises(ValueError, match="train_precision must be"):
        T.InversionTrainer(config(train_precision="bf16x3a"), cpu)
    assert set(tr.G.state_dict()) == set(T.InversionTrainer(config(), cpu).G.state_dict())  # a checkpoint does not know the arithmetic


def test_only_the_training_switch_takes_the_value():
    lib = _native.load_library()
    h = ctypes.c_void_p()
    cfg = _native.make_xfmr_config(O.BASE)
    _native.check(lib.hificar_xfmr_create(ctypes.byref(cfg), ctypes.byref(h)), "hificar_xfmr_create")
    WA = _native.PREC_BF16X3WA
    try:
        for p in (WA, _native.PREC_BF16X3W, WA, _native.PREC_BF16X3, WA, _native.PREC_F32, WA, WA):  # to and from every other training arithmetic
            assert lib.hificar_xfmr_set_train_precision(h, p) == 0
        for bad in (3, 5, 7, -1):
            assert lib.hificar_xfmr_set_train_precision(h, bad) == E_INVALID and b"precision" in lib.hificar_last_error()
        assert lib.hificar_xfmr_set_precision(h, WA) == E_INVALID and b"unknown precision 4" in lib.hificar_last_error()
        assert lib.hificar_xfmr_set_train_precision(h, _native.PREC_F32) == 0
        assert lib.hificar_xfmr_set_precision(h, _native.PREC_BF16X3) == 0  # an inference handle has no training arithmetic, this one neither
        assert lib.hificar_xfmr_set_train_precision(h, WA) == E_STATE and b"inference" in lib.hificar_last_error()
    finally:
        lib.hificar_xfmr_destroy(h)
    # the generator's config and switch (the conv engine's arithmetic)
    p = dict(E2W_PARAMS, use_tanh=True)
    bad = _native.make_config(p, WA)
    assert lib.hificar_create(ctypes.byref(bad), ctypes.byref(h)) == E_INVALID and b"unknown precision 4" in lib.hificar_last_error()
    ok = _native.make_config(p, _native.PREC_F32)
    _native.check(lib.hificar_create(ctypes.byref(ok), ctypes.byref(h)), "hificar_create")
    try:
        assert lib.hificar_set_precision(h, WA) == E_INVALID and b"unknown precision 4" in lib.hificar_last_error()
    finally:
        lib.hificar_destroy(h)
    header = open(os.path.join(REPO, "include", "hificar.h")).read()
    assert "#define HIFICAR_PREC_BF16X3WA 4 " in header
    assert "bf16 MFMAs in the attention" not in header
