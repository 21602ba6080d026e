"""The Transformer's opt-in bf16x3 arithmetic, as far as it goes without a device: the C ABI's precision switch on a created handle, the
Python surface (keyword, environment, training refusal, copies) and the CPU emulation that set the GPU tests' bar."""

import copy
import ctypes
import inspect
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_err
from transformer_bf16x3_emulation import Bf16x3Oracle
from transformer_oracle import TransformerOracle
from articulatory_amd import _native
from articulatory_amd.models import Transformer
from articulatory_amd.utils.synth import synth_transformer_state_dict, uniform

SMALL = dict(in_channels=12, out_channels=20, elayers=2, hidden_dim=128)
E_INVALID, E_STATE = -1, -2


def test_set_precision_on_a_created_handle():
    lib = _native.load_library()
    h = ctypes.c_void_p()
    cfg = _native.make_xfmr_config(SMALL)
    _native.check(lib.hificar_xfmr_create(ctypes.byref(cfg), ctypes.byref(h)), "hificar_xfmr_create")
    try:
        f32 = lib.hificar_xfmr_workspace_bytes(h, 3, 263)
        assert lib.hificar_xfmr_set_precision(h, _native.PREC_BF16X3) == 0
        x3 = lib.hificar_xfmr_workspace_bytes(h, 3, 263)
        assert lib.hificar_xfmr_set_precision(h, _native.PREC_F32) == 0
        assert lib.hificar_xfmr_workspace_bytes(h, 3, 263) == f32 > 0
        # two more row buffers [B T rounded up to 256][hidden_dim] of fp32-sized rows
        assert x3 - f32 == 2 * 1024 * SMALL["hidden_dim"] * 4
        assert lib.hificar_xfmr_set_precision(h, 7) == E_INVALID and b"precision" in lib.hificar_last_error()
        assert lib.hificar_xfmr_set_precision(h, -1) == E_INVALID
        assert lib.hificar_xfmr_set_precision(None, _native.PREC_F32) == E_INVALID
        assert lib.hificar_xfmr_workspace_bytes(h, 3, 263) == f32  # a refused value changes nothing
        # a bf16x3 handle refuses the "conv_blocks" tap (those rows exist as split rows only); an fp32 handle takes it
        dst = (ctypes.c_float * 4)()
        assert lib.hificar_xfmr_debug_tap(h, b"conv_blocks", dst, 4) == 0
        assert lib.hificar_xfmr_debug_tap(h, None, None, 0) == 0
        assert lib.hificar_xfmr_set_precision(h, _native.PREC_BF16X3) == 0
        assert lib.hificar_xfmr_debug_tap(h, b"conv_blocks", dst, 4) == E_INVALID and b"split" in lib.hificar_last_error()
        assert lib.hificar_xfmr_debug_tap(h, b"w_raw_in", dst, 4) == 0
    finally:
        lib.hificar_xfmr_destroy(h)


def test_precision_keyword_and_environment(monkeypatch):
    monkeypatch.setenv("HIFICAR_PRECISION", "bf16x3")
    assert Transformer(**SMALL).precision == "f32"  # the variable is the HiFi-GAN generators': not read here
    assert Transformer(**SMALL, precision=None).precision == "f32"
    assert Transformer(**SMALL, precision="bf16x3").precision == "bf16x3"
    for bad in ("fp16", "bf16", "", 1):
        with pytest.raises(ValueError, match="precision must be one of"):
            Transformer(**SMALL, precision=bad)
    m = Transformer(**SMALL)
    with pytest.raises(ValueError, match="precision must be one of"):
        m.set_precision("fp16")
    m.set_precision("bf16x3")
    assert m.precision == "bf16x3"
    assert "precision" not in inspect.signature(Transformer.__init__).parameters  # __init__ keeps the reference's signature


def test_training_is_refused_before_any_device_check():
    m = Transformer(**SMALL, precision="bf16x3").train()
    x = torch.zeros(2, SMALL["in_channels"], 16)
    for call in (lambda: m(x), lambda: m.forward_padded(x, [16, 9]), lambda: m.forward_padded(x, [16, 9], packed=True)):
        with pytest.raises(RuntimeError, match="training runs in the exact-fp32 arithmetic.*bf16x3"):
            call()
    m.set_precision("f32")
    with pytest.raises(NotImplementedError, match="CUDA/HIP"):  # the fp32 model gets as far as the device check
        m(x)


def test_copies_keep_the_precision():
    m = Transformer(**SMALL, precision="bf16x3")
    assert copy.deepcopy(m).precision == "bf16x3"
    assert pickle.loads(pickle.dumps(m)).precision == "bf16x3"
    assert m.__getstate__()["precision"] == "bf16x3"
    m.load_state_dict(Transformer(**SMALL).state_dict())
    assert m.precision == "bf16x3"
    assert "precision" not in m.state_dict()


def test_emulation_perturbs_the_result_and_stays_below_the_bar():
    """On the small golden model at T = 101 the emulated bf16x3 forward differs from the float64 restatement, by less than 1e-4 of max|y|:
    the condition under which the GPU tests' bar is the project's 2e-4."""
    gold = np.load(os.path.join(GOLDEN, "gold_transformer.npz"))
    cin, cout, elayers, hidden, seed = (int(v) for v in gold["small_params"])
    sd = synth_transformer_state_dict(dict(in_channels=cin, out_channels=cout, elayers=elayers, hidden_dim=hidden), seed=seed)
    x = uniform(seed, "x.101", (1, cin, 101), -1.0, 1.0)
    want = TransformerOracle(sd).forward(x).numpy()
    err = rel_err(Bf16x3Oracle(sd).forward(x).numpy(), want)
    print(f"emulated bf16x3 against float64, small T=101: {err:.3g}")
    assert 0.0 < err <= 1e-4 < 2e-4
    assert rel_err(want, gold["small_T101_y"]) < 2e-5  # (the restatement is the reference's function)
