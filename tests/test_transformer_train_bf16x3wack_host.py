"""The Transformer's opt-in bf16x3wack TRAINING arithmetic (bf16x3wac, and the attention's key-tiled backward — dK, dV, the tables' gradient — on
bf16 MFMAs too), as far as it goes without a device: the CPU emulation that set the GPU tests' bars
(tests/transformer_train_bf16x3wack_emulation.py) and what it moves against the bf16x3wac emulation, the Python surface, the trainer's config
key, the C ABI's switch and refusals, and the header line."""

import copy
import ctypes
import logging
import os
import pickle

import pytest
import torch

import transformer_ragged_oracle as R
import transformer_train_bf16x3_emulation as E
import transformer_train_bf16x3wa_emulation as EA
import transformer_train_bf16x3wac_emulation as EC
import transformer_train_bf16x3wack_emulation as EK
import transformer_train_oracle as O
from conftest import E2W_PARAMS, REPO
from test_transformer_train_host import config
from articulatory_amd import _native
from articulatory_amd.bin import train as T
from articulatory_amd.models import Transformer

E_INVALID, E_STATE = -1, -2
ATTENTION_INPUTS = ("self_attn.w_q", "self_attn.w_k", "self_attn.w_v", "self_attn.relative_positional.embeddings")


# ------------------------------------------------------------------------------------------------ the emulation and its bars
@pytest.fixture(scope="module")
def emulated():
    return EK.emulated_errors(verbose=True)


def test_recorded_bars_follow_the_rule():
    for k, e in EK.EMULATED.items():
        want = E.X3_OUT_BAR if k == "out" else (EC.BARS_X3WAC[k] if e <= EC.BARS_X3WAC[k] / 4 else 4 * e)
        assert EK.BARS_X3WACK[k] == want, k
    assert set(EK.EMULATED) == set(EC.EMULATED) == set(EK.BARS_X3WACK)
    assert 0 < EK.EMULATED["out"] < 1e-4 and EK.BARS_X3WACK["out"] == 2e-4 < E.NORTH_STAR_TOL
    assert all(EK.BARS_X3WACK[k] >= EC.BARS_X3WAC[k] for k in EK.BARS_X3WACK)  # never tighter than the arithmetic it extends
    # the GPU cases, all of them: head size 16 at the tile and band edges, one case per template instantiation, the ragged four
    assert EK.DENSE_CASES == ("t2", "t65", "t101", "t200", "t263", "b1", "t330")
    assert EK.HEAD_CASES == tuple(f"d{d}" for d in range(32, 129, 16))
    assert set(EK.ALL_DENSE) <= set(O.SHAPES) | set(O.EDGE_SHAPES) and EK.RAGGED_CASES == ("mixed", "tiles", "band", "zero")
    assert set(EK.RAGGED_CASES) <= set(R.RAGGED_SHAPES)
    heads = lambda name: (O.EDGE_SHAPES.get(name) or O.SHAPES[name])[0]["hidden_dim"] // 8  # noqa: E731
    assert {heads(n) for n in EK.DENSE_CASES} == {16} and [heads(n) for n in EK.HEAD_CASES] == list(range(32, 129, 16))


def test_emulated_errors_are_below_a_quarter_of_the_bars(emulated):
    worst, gap = emulated
    assert set(worst) == set(EK.BARS_X3WACK)
    for k, e in sorted(worst.items()):
        print(f"  {k}: emulated {e:.3g}, recorded {EK.EMULATED[k]:g}, device bar {EK.BARS_X3WACK[k]:g}")
        assert 0 < e <= EK.EMULATED[k] and e <= EK.BARS_X3WACK[k] / 4, k
    assert gap < E.X3_OUT_BAR  # the forward is bf16x3wa's: the ReLU-side condition holds as it does there


@pytest.mark.parametrize("name", ["t65", "d48"])
def test_the_emulation_reroutes_the_key_tiled_products_and_nothing_else(name):
    """Against the bf16x3wac emulation on the same case: out, loss, statistics, running buffers and everything above the attention of the last
    layer (its w_o, norms, feed-forward, w_out) are equal to the bit, and so is the last layer's w_q gradient, which sees the attention's
    backward through dQ alone; the last layer's w_k, w_v and table gradients move, by rounding: they stay within a quarter of the bar."""
    shapes = O.EDGE_SHAPES if name in O.EDGE_SHAPES else None
    with EC.emulating():
        a = O.restatement(name, torch.float64, shapes=shapes)
    with EK.emulating():
        b = O.restatement(name, torch.float64, shapes=shapes)
    assert O.banded_attention_train is EA._attention and O.F is torch.nn.functional  # (the reroutes are undone)
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["stats"], b["stats"]) and float(a["loss"]) == float(b["loss"])
    assert all(torch.equal(a["running"][k], v) for k, v in b["running"].items())
    assert not torch.equal(a["dx"], b["dx"])
    last = f"transformer.layers.{(shapes or O.SHAPES)[name][0]['elayers'] - 1}."
    moved = {k for k in a["grads"] if not torch.equal(a["grads"][k], b["grads"][k])}
    assert {last + t for t in ATTENTION_INPUTS[1:]} <= moved
    assert not any(k.startswith(last) or k.startswith("w_out") for k in moved - {last + t for t in ATTENTION_INPUTS[1:]}), sorted(moved)
    assert last + "self_attn.w_q" not in moved
    ref = O.restatement(name, torch.float64, gates=b["sides"], shapes=shapes)
    for k in moved:
        assert float((b["grads"][k] - ref["grads"][k]).abs().max()) / O.grad_scale(ref["grads"], k) < EK.BARS_X3WACK["grad"] / 4, k


def test_the_split_products_are_what_the_docstring_says():
    """dK, dV and dE of the emulated attention against the three terms written out, and against the exact products of the same dS and Pd."""
    torch.manual_seed(5)
    B, H, Tn, d = 1, 2, 7, 16
    q, k, v = (torch.randn(B, H, Tn, d, dtype=torch.float64, requires_grad=True) for _ in range(3))
    emb = torch.randn(H, EK.TAB, d, dtype=torch.float64, requires_grad=True)
    do = torch.randn(B, H, Tn, d, dtype=torch.float64)
    ga = torch.autograd.grad(EA.attention3(q, k, v, emb), (q, k, v, emb), do)
    gk = torch.autograd.grad(EK.attention3k(q, k, v, emb), (q, k, v, emb), do)
    assert torch.equal(ga[0], gk[0])  # dQ is bf16x3wa's statement
    for exact, split3 in zip(ga[1:], gk[1:]):
        rel = float((exact - split3).abs().max() / exact.abs().max())
        assert 0 < rel < 3 * 2.0 ** -16  # lo lo is dropped, and each lo is rounded to 8 bits: a few 2^-17 of the largest term


# ------------------------------------------------------------------------------------------------ the Python surface and the C ABI
def test_keyword_setter_copies_and_refusals():
    assert _native.PREC_BF16X3WACK == 8 and _native.XFMR_TRAIN_PRECISIONS_K == dict(_native.XFMR_TRAIN_PRECISIONS_ALL, bf16x3wack=8)
    assert _native.TRAIN_PRECISIONS == {"f32": 0, "bf16x3": 1, "bf16x3w": 2} and _native.XFMR_TRAIN_PRECISIONS == dict(_native.TRAIN_PRECISIONS, bf16x3wa=4)
    assert _native.XFMR_TRAIN_PRECISIONS_ALL == dict(_native.XFMR_TRAIN_PRECISIONS, bf16x3wac=6)
    assert "bf16x3wack" not in _native.XFMR_PRECISIONS
    m = Transformer(train_precision="bf16x3wack", **O.BASE)
    assert m.train_precision == "bf16x3wack" and m.precision == "f32"
    assert copy.deepcopy(m).train_precision == "bf16x3wack" and pickle.loads(pickle.dumps(m)).train_precision == "bf16x3wack"
    assert not any("precision" in k for k in m.state_dict())
    for to in ("bf16x3wac", "bf16x3wa", "bf16x3w", "bf16x3", "f32", "bf16x3wack"):  # (no handle yet: the choice alone)
        m.set_train_precision(to)
        assert m.train_precision == to
    # the inference arithmetic does not know the value
    with pytest.raises(ValueError, match="precision must be one of"):
        Transformer(precision="bf16x3wack", **O.BASE)
    with pytest.raises(ValueError, match="precision must be one of"):
        Transformer(**O.BASE).set_precision("bf16x3wack")
    for inference in ("bf16x3", "bf16x3a"):
        with pytest.raises(ValueError, match="inference-only"):
            Transformer(precision=inference, train_precision="bf16x3wack", **O.BASE)
        with pytest.raises(ValueError, match="inference-only"):
            Transformer(precision=inference, **O.BASE).set_train_precision("bf16x3wack")
        with pytest.raises(ValueError, match="inference-only"):
            m.set_precision(inference)
    for bad in ("bf16x3WACK", "bf16x3wak", "bf16x3wck", "bf16x3k", 8):
        with pytest.raises(ValueError, match="train_precision must be one of"):
            Transformer(train_precision=bad, **O.BASE)
        with pytest.raises(ValueError, match="train_precision must be one of"):
            Transformer(**O.BASE).set_train_precision(bad)
    with pytest.raises(NotImplementedError, match="on the device only"):
        Transformer(train_precision="bf16x3wack", **O.BASE).train()(torch.zeros(2, 12, 5))


def test_the_trainer_reads_the_config_key(caplog):
    cpu = torch.device("cpu")
    with caplog.at_level(logging.INFO):
        tr = T.InversionTrainer(config(train_precision="bf16x3wack"), cpu)
    assert tr.G.train_precision == "bf16x3wack" and tr.G.precision == "f32" and tr.train_precision == "bf16x3wack"
    assert "training arithmetic bf16x3wack" in caplog.records[0].getMessage()
    bigru = dict(config(), generator_type="BiGRU", generator_params=dict(in_channels=12, out_channels=8))
    with pytest.raises(NotImplementedError, match="train_precision bf16x3wack is built for generator_type Transformer"):
        T.InversionTrainer(dict(bigru, train_precision="bf16x3wack"), cpu)
    with pytest.raises(ValueError, match="train_precision must be"):
        T.InversionTrainer(config(train_precision="bf16x3wak"), cpu)
    assert set(tr.G.state_dict()) == set(T.InversionTrainer(config(), cpu).G.state_dict())  # a checkpoint does not know the arithmetic


def test_only_the_training_switch_takes_the_value():
    lib = _native.load_library()
    h = ctypes.c_void_p()
    cfg = _native.make_xfmr_config(O.BASE)
    _native.check(lib.hificar_xfmr_create(ctypes.byref(cfg), ctypes.byref(h)), "hificar_xfmr_create")
    K = _native.PREC_BF16X3WACK
    try:
        # to and from every other training arithmetic
        for p in (K, _native.PREC_BF16X3WAC, K, _native.PREC_BF16X3WA, K, _native.PREC_BF16X3W, K, _native.PREC_BF16X3, K, _native.PREC_F32, K, K):
            assert lib.hificar_xfmr_set_train_precision(h, p) == 0
        for bad in (3, 5, 7, 9, -1):
            assert lib.hificar_xfmr_set_train_precision(h, bad) == E_INVALID and b"precision" in lib.hificar_last_error()
        assert lib.hificar_xfmr_set_precision(h, K) == E_INVALID and b"unknown precision 8" in lib.hificar_last_error()
        assert lib.hificar_xfmr_set_train_precision(h, _native.PREC_F32) == 0
        for inference in (_native.PREC_BF16X3, _native.PREC_BF16X3A):  # an inference handle has no training arithmetic, this one neither
            assert lib.hificar_xfmr_set_precision(h, inference) == 0
            assert lib.hificar_xfmr_set_train_precision(h, K) == E_STATE and b"inference" in lib.hificar_last_error()
    finally:
        lib.hificar_xfmr_destroy(h)
    # the generator's config and switch (the conv engine's arithmetic)
    p = dict(E2W_PARAMS, use_tanh=True)
    bad = _native.make_config(p, K)
    assert lib.hificar_create(ctypes.byref(bad), ctypes.byref(h)) == E_INVALID and b"unknown precision 8" in lib.hificar_last_error()
    ok = _native.make_config(p, _native.PREC_F32)
    _native.check(lib.hificar_create(ctypes.byref(ok), ctypes.byref(h)), "hificar_create")
    try:
        assert lib.hificar_set_precision(h, K) == E_INVALID and b"unknown precision 8" in lib.hificar_last_error()
    finally:
        lib.hificar_destroy(h)
    header = open(os.path.join(REPO, "include", "hificar.h")).read()
    assert "#define HIFICAR_PREC_BF16X3WACK 8 " in header
    assert "dK / dV / the table gradient on bf16 MFMAs" not in header  # (no longer among the "Not built")
