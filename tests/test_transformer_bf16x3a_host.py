"""The Transformer's opt-in bf16x3a arithmetic (bf16x3, and the attention's products on bf16 MFMAs too), as far as it goes without a device:
the C ABI's fourth precision value on a created handle, the Python surface, and the CPU emulation that set the GPU tests' bar."""

import copy
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import E2W_PARAMS, GOLDEN, REPO, rel_err
from transformer_bf16x3_emulation import Bf16x3Oracle
from transformer_bf16x3a_emulation import PEAKED_GAIN, Bf16x3aOracle, peaked_state_dict
from transformer_oracle import TransformerOracle
from articulatory_amd import _native
from articulatory_amd.bin import decode as D
from articulatory_amd.models import HiFiGANGenerator, Transformer
from articulatory_amd.utils.synth import synth_transformer_state_dict, uniform

SMALL = dict(in_channels=12, out_channels=20, elayers=2, hidden_dim=128)
E_INVALID, E_STATE = -1, -2


def test_the_value_and_the_tables_of_names():
    assert _native.PREC_BF16X3A == 3
    assert "#define HIFICAR_PREC_BF16X3A 3 " in open(os.path.join(REPO, "include", "hificar.h")).read()
    assert _native.XFMR_PRECISIONS == {"f32": 0, "bf16x3": 1, "bf16x3a": 3}
    # what the other models validate against is unchanged
    assert _native.PRECISIONS == {"f32": 0, "bf16x3": 1}
    assert _native.TRAIN_PRECISIONS == {"f32": 0, "bf16x3": 1, "bf16x3w": 2}


def test_set_precision_on_a_created_handle():
    lib = _native.load_library()
    h = ctypes.c_void_p()
    cfg = _native.make_xfmr_config(SMALL)
    _native.check(lib.hificar_xfmr_create(ctypes.byref(cfg), ctypes.byref(h)), "hificar_xfmr_create")
    try:
        f32 = lib.hificar_xfmr_workspace_bytes(h, 3, 263)
        assert lib.hificar_xfmr_set_precision(h, _native.PREC_BF16X3) == 0
        x3 = lib.hificar_xfmr_workspace_bytes(h, 3, 263)
        assert lib.hificar_xfmr_set_precision(h, _native.PREC_BF16X3A) == 0
        assert lib.hificar_xfmr_workspace_bytes(h, 3, 263) == x3 > f32 > 0  # the same five row buffers
        for bad in (_native.PREC_BF16X3W, 5, 7, 9, -1):  # (5, 7: the gaps in the values; the other training values: their own host tests)
            assert lib.hificar_xfmr_set_precision(h, bad) == E_INVALID and b"unknown precision" in lib.hificar_last_error()
        assert lib.hificar_xfmr_workspace_bytes(h, 3, 263) == x3  # a refused value changes nothing
        dst = (ctypes.c_float * 4)()
        assert lib.hificar_xfmr_debug_tap(h, b"conv_blocks", dst, 4) == E_INVALID and b"split" in lib.hificar_last_error()
        assert lib.hificar_xfmr_debug_tap(h, b"w_raw_in", dst, 4) == 0
        assert lib.hificar_xfmr_debug_tap(h, None, None, 0) == 0
        # an inference handle has no training arithmetic
        assert lib.hificar_xfmr_set_train_precision(h, _native.PREC_BF16X3) == E_STATE and b"inference" in lib.hificar_last_error()
        assert b"bf16x3a" in lib.hificar_last_error()
        assert lib.hificar_xfmr_set_precision(h, _native.PREC_F32) == 0
        assert lib.hificar_xfmr_workspace_bytes(h, 3, 263) == f32
        assert lib.hificar_xfmr_set_train_precision(h, _native.PREC_BF16X3A) == E_INVALID  # not a training arithmetic
    finally:
        lib.hificar_xfmr_destroy(h)


def test_the_generators_refuse_the_value():
    lib = _native.load_library()
    h = ctypes.c_void_p()
    p = dict(E2W_PARAMS, use_tanh=True)
    bad = _native.make_config(p, _native.PREC_BF16X3A)
    assert lib.hificar_create(ctypes.byref(bad), ctypes.byref(h)) == E_INVALID and b"unknown precision 3" in lib.hificar_last_error()
    ok = _native.make_config(p, _native.PREC_F32)
    _native.check(lib.hificar_create(ctypes.byref(ok), ctypes.byref(h)), "hificar_create")
    try:
        assert lib.hificar_set_precision(h, _native.PREC_BF16X3A) == E_INVALID and b"unknown precision 3" in lib.hificar_last_error()
    finally:
        lib.hificar_destroy(h)
    with pytest.raises(ValueError, match="precision must be one of"):
        HiFiGANGenerator(**E2W_PARAMS, precision="bf16x3a")


def test_precision_keyword_setter_and_environment(monkeypatch):
    monkeypatch.setenv("HIFICAR_PRECISION", "bf16x3a")
    assert Transformer(**SMALL).precision == "f32"  # the variable is the HiFi-GAN generators': not read here
    assert Transformer(**SMALL, precision="bf16x3a").precision == "bf16x3a"
    m = Transformer(**SMALL)
    for to in ("bf16x3a", "bf16x3", "bf16x3a", "f32"):
        m.set_precision(to)
        assert m.precision == to
    for bad in ("bf16x3A", "bf16a", 3):
        with pytest.raises(ValueError, match="^precision must be one of"):
            Transformer(**SMALL, precision=bad)
        with pytest.raises(ValueError, match="^precision must be one of"):
            m.set_precision(bad)
    # inference only, in every combination
    with pytest.raises(ValueError, match="inference-only"):
        Transformer(**SMALL, precision="bf16x3a", train_precision="bf16x3")
    with pytest.raises(ValueError, match="inference-only"):
        Transformer(**SMALL, precision="bf16x3a").set_train_precision("bf16x3w")
    with pytest.raises(ValueError, match="inference-only"):
        Transformer(**SMALL, train_precision="bf16x3").set_precision("bf16x3a")
    with pytest.raises(ValueError, match="train_precision must be one of"):
        Transformer(**SMALL, train_precision="bf16x3a")


def test_training_is_refused_before_any_device_check():
    m = Transformer(**SMALL, precision="bf16x3a").train()
    x = torch.zeros(2, SMALL["in_channels"], 16)
    for call in (lambda: m(x), lambda: m.forward_padded(x, [16, 9]), lambda: m.forward_padded(x, [16, 9], packed=True)):
        with pytest.raises(RuntimeError, match="training runs in the exact-fp32 arithmetic.*bf16x3a"):
            call()


def test_copies_keep_the_precision():
    m = Transformer(**SMALL, precision="bf16x3a")
    assert copy.deepcopy(m).precision == "bf16x3a"
    assert pickle.loads(pickle.dumps(m)).precision == "bf16x3a"
    m.load_state_dict(Transformer(**SMALL).state_dict())
    assert m.precision == "bf16x3a"
    assert not any("precision" in k for k in m.state_dict())


def test_decode_takes_the_flag():
    assert D.get_parser().parse_args(["--precision", "bf16x3a"] + _decode_required()).precision == "bf16x3a"


def _decode_required():
    return ["--checkpoint", "x.pkl", "--outdir", "out"]


@pytest.mark.parametrize("case", ["small_T101", "wq_gain4_T260"])
def test_emulation_perturbs_the_result_and_stays_below_the_bar(case):
    """The emulated bf16x3a forward differs from the float64 restatement and from the emulated bf16x3 forward, and stays within 1e-4 of
    max|y|: the condition under which the GPU tests' bar is the project's 2e-4.  The second case is the peaked softmax:
    every self_attn.w_q of the small golden model times 4."""
    gold = np.load(os.path.join(GOLDEN, "gold_transformer.npz"))
    cin, cout, elayers, hidden, seed = (int(v) for v in gold["small_params"])
    sd = synth_transformer_state_dict(dict(in_channels=cin, out_channels=cout, elayers=elayers, hidden_dim=hidden), seed=seed)
    T = 101 if case == "small_T101" else 260
    if case != "small_T101":
        sd = peaked_state_dict(sd, PEAKED_GAIN)
    x = uniform(seed, f"x.{T}", (1, cin, T), -1.0, 1.0)
    want = TransformerOracle(sd).forward(x).numpy()
    got = Bf16x3aOracle(sd).forward(x).numpy()
    err = rel_err(got, want)
    print(f"emulated bf16x3a against float64, {case}: {err:.3g}")
    assert 0.0 < err <= 1e-4 < 2e-4
    assert not np.array_equal(got, Bf16x3Oracle(sd).forward(x).numpy())
