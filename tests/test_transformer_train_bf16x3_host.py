"""The Transformer's opt-in bf16x3 TRAINING arithmetic, as far as it goes without a device: the CPU emulation that set the GPU tests' bars
(tests/transformer_train_bf16x3_emulation.py), the Python surface (keyword, copies, refusals), the C ABI's switch on a created handle, the
trainer's config key, and the device weight pack's index arithmetic run on the host against a restatement of the host pack."""

import copy
import ctypes
import inspect
import logging
import pickle

import numpy as np
import pytest
import torch

import transformer_train_bf16x3_emulation as E
import transformer_train_oracle as O
from test_transformer_train_host import config
from articulatory_amd import _native
from articulatory_amd.bin import train as T
from articulatory_amd.models import Transformer
from articulatory_amd.utils.synth import uniform

E_INVALID, E_STATE = -1, -2


@pytest.fixture(scope="module")
def emulated():
    return E.emulated_errors(verbose=True)


def test_recorded_bars_follow_the_rule():
    for k, e in E.EMULATED.items():
        want = E.X3_OUT_BAR if k == "out" else (E.FP32_BARS[k] if e <= E.FP32_BARS[k] / 4 else 4 * e)
        assert E.BARS_X3[k] == want, k
    assert E.EMULATED["out"] < 1e-4 and E.BARS_X3["out"] == 2e-4 < E.NORTH_STAR_TOL
    assert set(E.CASES) <= set(O.SHAPES)


def test_emulated_errors_are_below_a_quarter_of_the_bars(emulated):
    worst, _ = emulated
    assert set(worst) == set(E.BARS_X3)
    for k, e in sorted(worst.items()):
        print(f"  {k}: emulated {e:.3g}, recorded {E.EMULATED[k]:g}, device bar {E.BARS_X3[k]:g}")
        assert 0 < e <= E.EMULATED[k] and e <= E.BARS_X3[k] / 4, k
    # the arithmetic is not exact fp32: the emulation moves the output by more than the fp32 suite's own float32 run does (1e-6)
    assert worst["out"] > 5e-6


def test_emulated_gate_flips_lie_within_the_output_bar_of_zero(emulated):
    _, gap = emulated
    assert gap < E.X3_OUT_BAR


def test_keyword_copies_and_refusals():
    m = Transformer(**O.BASE)
    assert m.train_precision == "f32" and Transformer(train_precision=None, **O.BASE).train_precision == "f32"
    m = Transformer(train_precision="bf16x3", **O.BASE)
    assert m.train_precision == "bf16x3" and m.precision == "f32"
    for bad in ("bf16", "fp32", 1):
        with pytest.raises(ValueError, match="train_precision"):
            Transformer(train_precision=bad, **O.BASE)
        with pytest.raises(ValueError, match="train_precision"):
            m.set_train_precision(bad)
    with pytest.raises(ValueError, match="inference-only"):
        Transformer(precision="bf16x3", train_precision="bf16x3", **O.BASE)
    with pytest.raises(ValueError, match="inference-only"):
        m.set_precision("bf16x3")
    with pytest.raises(ValueError, match="inference-only"):
        Transformer(precision="bf16x3", **O.BASE).set_train_precision("bf16x3")
    Transformer(precision="bf16x3", train_precision="f32", **O.BASE)
    assert "train_precision" not in inspect.signature(Transformer.__init__).parameters
    assert not any("precision" in k for k in m.state_dict())
    assert copy.deepcopy(m).train_precision == "bf16x3" and pickle.loads(pickle.dumps(m)).train_precision == "bf16x3"
    m.set_train_precision("f32")  # (no handle yet: the choice alone)
    assert m.train_precision == "f32" and copy.deepcopy(m).train_precision == "f32"
    # the train()-mode refusals that need no device stay what they were
    with pytest.raises(RuntimeError, match="exact-fp32"):
        Transformer(precision="bf16x3", **O.BASE).train()(torch.zeros(2, 12, 5))
    with pytest.raises(NotImplementedError, match="on the device only"):
        Transformer(train_precision="bf16x3", **O.BASE).train()(torch.zeros(2, 12, 5))


def test_set_train_precision_on_a_created_handle():
    lib = _native.load_library()
    h = ctypes.c_void_p()
    cfg = _native.make_xfmr_config(O.BASE)
    _native.check(lib.hificar_xfmr_create(ctypes.byref(cfg), ctypes.byref(h)), "hificar_xfmr_create")
    try:
        assert lib.hificar_xfmr_set_train_precision(h, _native.PREC_BF16X3) == 0
        assert lib.hificar_xfmr_set_train_precision(h, _native.PREC_F32) == 0
        for bad in (7, -1):
            assert lib.hificar_xfmr_set_train_precision(h, bad) == E_INVALID and b"precision" in lib.hificar_last_error()
        assert lib.hificar_xfmr_set_train_precision(None, _native.PREC_F32) == E_INVALID
        assert lib.hificar_xfmr_set_precision(h, _native.PREC_BF16X3) == 0
        for p in (_native.PREC_F32, _native.PREC_BF16X3):
            assert lib.hificar_xfmr_set_train_precision(h, p) == E_STATE and b"inference" in lib.hificar_last_error()
        assert lib.hificar_xfmr_set_train_precision(h, 7) == E_INVALID
        assert lib.hificar_xfmr_set_precision(h, _native.PREC_F32) == 0
        assert lib.hificar_xfmr_set_train_precision(h, _native.PREC_BF16X3) == 0
        # the tape does not depend on the arithmetic, and nothing here needed a device (the handle is not finalized: no tape yet)
        assert lib.hificar_xfmr_tape_bytes(h, 2, 100) == 0
    finally:
        lib.hificar_xfmr_destroy(h)


def test_the_trainer_reads_the_config_key(caplog):
    cpu = torch.device("cpu")
    assert T.InversionTrainer(config(), cpu).G.train_precision == "f32"
    with caplog.at_level(logging.INFO):
        tr = T.InversionTrainer(config(train_precision="bf16x3"), cpu)
    assert tr.G.train_precision == "bf16x3" and tr.G.precision == "f32" and tr.train_precision == "bf16x3"
    assert "training arithmetic bf16x3" in caplog.records[0].getMessage()
    with pytest.raises(ValueError, match="train_precision"):
        T.InversionTrainer(config(train_precision="bf16"), cpu)
    bigru = dict(config(), generator_type="BiGRU", generator_params=dict(in_channels=12, out_channels=8))
    with pytest.raises(NotImplementedError, match="train_precision bf16x3 is built for generator_type Transformer"):
        T.InversionTrainer(dict(bigru, train_precision="bf16x3"), cpu)
    # a checkpoint does not know the arithmetic
    assert set(tr.G.state_dict()) == set(T.InversionTrainer(config(), cpu).G.state_dict())


# ------------------------------------------------------------------------------------------------ the device pack's index arithmetic
def bf16(a):
    """float32 array -> its bf16 bits, round to nearest even (finite values)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def host_pack(w, cin_pad):
    """The fragments of a Conv1d weight w (cout, cin, K) as the host pack of the inference handles lays them out, restated from the layout's
    definition: [n_block32][chunk][tap][c16][hi | lo][lane][8] with lane = (g = lane >> 5, n = lane & 31) holding channels
    c chunk + 16 u + 8 g + j of output channel 32 nb + n, hi = bf16(w), lo = bf16(w - hi), and a zero tail of 4 nc16 fragments."""
    cout, cin, K = w.shape
    chunk = 64 if cin_pad % 64 == 0 and cin_pad >= 128 else 32 if cin_pad % 32 == 0 and cin_pad >= 64 else 16
    nb32, nchunk, nc16 = (cout + 31) // 32, cin_pad // chunk, chunk // 16
    full = np.zeros((nb32 * 32, cin_pad, K), np.float32)
    full[:cout, :cin] = w
    hi = bf16(full)
    lo = bf16(full - (hi.astype(np.uint32) << 16).view(np.float32))
    out = np.zeros((nb32, nchunk, K, nc16, 2, 64, 8), np.uint16)
    for half, src in enumerate((hi, lo)):
        s = src.reshape(nb32, 32, nchunk, nc16, 2, 8, K)            # [nb][n][c][u][g][j][t]
        out[:, :, :, :, half] = s.transpose(0, 2, 6, 3, 4, 1, 5).reshape(nb32, nchunk, K, nc16, 64, 8)  # lane = 32 g + n
    return np.concatenate([out.reshape(-1), np.zeros(4 * nc16 * 512, np.uint16)])


def device_pack(w, cin_pad, mode, how):
    lib = _native.load_library()
    cout, cin, K = w.shape
    w = np.ascontiguousarray(w, dtype=np.float32)
    n = ctypes.c_size_t()
    assert lib.hificar_debug_pack16(cout, cin, cin_pad, K, mode, how, w.ctypes.data, None, 0, ctypes.byref(n)) == E_INVALID  # (null buffer)
    probe = np.zeros(1, np.uint16)
    assert lib.hificar_debug_pack16(cout, cin, cin_pad, K, mode, how, w.ctypes.data, probe.ctypes.data, 1, ctypes.byref(n)) == E_INVALID and n.value > 1
    out = np.full(n.value, 0xABCD, np.uint16)
    _native.check(lib.hificar_debug_pack16(cout, cin, cin_pad, K, mode, how, w.ctypes.data, out.ctypes.data, out.size, ctypes.byref(n)), "hificar_debug_pack16")
    return out


PACK_LAYERS = [("conv1 of block 0", 128, 12, 32, 3, 0), ("q | k | v", 384, 128, 128, 1, 0), ("w_out", 40, 128, 128, 1, 0),
               ("conv1 of block 0, data gradient", 128, 12, 32, 3, 2), ("linear2, data gradient", 128, 3072, 3072, 1, 2), ("k = 3 at 64 channels", 64, 64, 64, 3, 0)]


@pytest.mark.parametrize("what,cout,cin,cin_pad,K,mode", PACK_LAYERS, ids=[p[0] for p in PACK_LAYERS])
def test_device_pack_index_arithmetic_gives_the_host_packs_bytes(what, cout, cin, cin_pad, K, mode):
    """hificar_debug_pack16 `how` 0 runs pack16_kernel's own index functions (hificar_xfmr_pack16.hip.h) over every work item on the host."""
    w = uniform(9100 + cout + cin, "pack", (cout, cin, K), -1.0, 1.0)
    w.reshape(-1)[:3] = (0.0, 1.0, -2.0 ** -20)
    got = device_pack(w, cin_pad, mode, 0)
    # mode 2: the data gradient's Conv1d, (cin -> its input channels): w'[ci][co][t] = w[co][ci][K - 1 - t], rows cout rounded up to 32 wide
    want = host_pack(w, cin_pad) if mode == 0 else host_pack(np.ascontiguousarray(w.transpose(1, 0, 2)[:, :, ::-1]), (cout + 31) // 32 * 32)
    assert got.size == want.size and np.array_equal(got, want)
    assert len(np.unique(got)) > 100  # (not a pack of zeros)
