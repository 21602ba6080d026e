"""The Transformer's opt-in bf16x3wac TRAINING arithmetic (bf16x3wa, and the weight gradients of the wide k = 3 convs on bf16 MFMAs too), as far as
it goes without a device: the tap-column split's layout from the library's host entry against a numpy restatement, the CPU emulation that set
the GPU tests' bars (tests/transformer_train_bf16x3wac_emulation.py) and what it moves against the bf16x3wa emulation, the restated selection
rule and launches (tests/transformer_bf16x3wac_forms.py), the Python surface, the trainer's config key and the C ABI's refusals."""

import copy
import ctypes
import logging
import os
import pickle

import numpy as np
import pytest
import torch

import transformer_bf16x3w_forms as W
import transformer_bf16x3wac_forms as WC
import transformer_ragged_oracle as R
import transformer_train_bf16x3_emulation as E
import transformer_train_bf16x3w_emulation as EW
import transformer_train_bf16x3wa_emulation as EA
import transformer_train_bf16x3wac_emulation as EC
import transformer_train_oracle as O
from conftest import E2W_PARAMS, REPO
from test_transformer_train_bf16x3w_host import SPLIT_PACKED, SPLIT_RAGGED, ragged_valid
from test_transformer_train_host import config
from articulatory_amd import _native
from articulatory_amd.bin import train as T
from articulatory_amd.models import Transformer
from articulatory_amd.utils.synth import uniform

E_INVALID, E_STATE = -1, -2


# ------------------------------------------------------------------------------------------------ the tap-column split's layout
def library_split(x, how, T=0, lengths=None, pad_row=None):
    """hificar_debug_split_taps_t's bytes (how 0: the device pass's index functions on the host; 1: the device pass)."""
    lib = _native.load_library()
    M, C = x.shape
    x = np.ascontiguousarray(x, dtype=np.float32)
    lens = None if lengths is None else np.asarray(lengths, dtype=np.int32)
    pads = None if pad_row is None else np.asarray(pad_row, dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    n = ctypes.c_size_t(0)
    probe = np.zeros(1, dtype=np.uint8)
    assert lib.hificar_debug_split_taps_t(M, C, T, ptr(lens), ptr(pads), how, x.ctypes.data, probe.ctypes.data, 1, ctypes.byref(n)) == E_INVALID
    assert n.value == (M + 7) // 8 * 3 * C * 32
    out = np.full(n.value + 64, 0xA5, dtype=np.uint8)
    _native.check(lib.hificar_debug_split_taps_t(M, C, T, ptr(lens), ptr(pads), how, x.ctypes.data, out.ctypes.data, n.value, ctypes.byref(n)),
                  "hificar_debug_split_taps_t")
    assert (out[n.value:] == 0xA5).all()  # nothing behind the split is written
    return out[:n.value]


def split_cases(how):
    """(what, the library's bytes, the numpy restatement's).  One sequence of M rows: the groups' edges, every width class; dense batches whose
    sequence boundaries fall at offsets 0, 1 and 7 of a group; a ragged and a packed batch with NaN in the rows that must not be read."""
    for M in (1, 7, 8, 9, 257):
        for C in (128, 384, 1024):
            x = uniform(9400 + M + C, "taps", (M, C), -1.0, 1.0)
            yield f"{M}x{C}", library_split(x, how), WC.split_taps_t(x)
    for B, T_ in ((8, 1), (9, 2), (3, 9)):  # T = 1: every frame is first and last; T = 2: boundaries at every even offset; T = 9: at offsets 1 and 2 (rows 9, 18)
        x = uniform(9410 + T_, "taps.dense", (B * T_, 128), -1.0, 1.0)
        yield f"dense {B}x{T_}", library_split(x, how, T=T_), WC.split_taps_t(x, T=T_)
    x = uniform(9420, "taps.dense", (5 * 3, 128), -1.0, 1.0)  # T = 3: a boundary at row 15, offset 7 of its group, and at offset 0 of none but the first: row 24 is past M
    yield "dense 5x3", library_split(x, how, T=3), WC.split_taps_t(x, T=3)
    x = uniform(9421, "taps.dense", (2 * 8, 128), -1.0, 1.0)  # T = 8: a boundary at offset 0 of the second group
    yield "dense 2x8", library_split(x, how, T=8), WC.split_taps_t(x, T=8)
    nan = np.float32("nan")
    T_, lengths = SPLIT_RAGGED["T"], SPLIT_RAGGED["lengths"]
    valid = ragged_valid(lengths, T_)
    x = uniform(9401, "taps.ragged", (valid.size, 128), -1.0, 1.0)
    x[~valid] = nan  # (rows of padded frames are not read)
    yield "ragged", library_split(x, how, T=T_, lengths=lengths), WC.split_taps_t(x, T=T_, valid=valid)
    valid = np.asarray(SPLIT_PACKED) >= 0
    x = uniform(9402, "taps.packed", (valid.size, 384), -1.0, 1.0)
    x[~valid] = nan
    yield "packed", library_split(x, how, pad_row=SPLIT_PACKED), WC.split_taps_t(x, valid=valid, packed=True)


N_SPLIT_CASES = 15 + 5 + 2


def test_tap_column_layout_on_the_host_is_the_numpy_restatement():
    """xfmr_split_taps_t_kernel's index functions, run on the host over a 0xFF-filled buffer, against the layout's definition."""
    seen = 0
    for what, got, want in split_cases(0):
        assert got.shape == want.shape and np.array_equal(got, want), what
        assert not np.array_equal(got, np.zeros_like(got)), what
        seen += 1
    assert seen == N_SPLIT_CASES


def test_tap_column_restatement_is_the_definition_element_by_element():
    """The numpy restatement itself against the scalar definition: (row r, tap k, channel c) -> bytes ((r // 8) 3 C + k C + c) 32 + 2 (r % 8),
    lo 16 further; the value is row r + k - 1's where that is a frame of row r's sequence."""
    T_, C = 4, 128
    x = uniform(9403, "taps.def", (12, C), -1.0, 1.0)
    valid = np.ones(12, dtype=bool)
    valid[6:8] = False  # the second sequence has two frames
    x[~valid] = np.float32("nan")
    b = WC.split_taps_t(x, T=T_, valid=valid).view(np.uint16)
    assert b.size == 2 * 3 * C * 16
    for r in range(16):
        for k in range(3):
            for c in (0, 31, 127):
                at = ((r // 8) * 3 * C + k * C + c) * 16 + r % 8
                s = r + k - 1
                if r >= 12 or not 0 <= s < 12 or not valid[s] or s // T_ != r // T_:
                    assert b[at] == 0 and b[at + 8] == 0, (r, k, c)
                    continue
                hi = W.bf16(x[s:s + 1, c])[0]
                lo = W.bf16(x[s:s + 1, c] - (np.uint32(hi) << 16).view(np.float32))[0]
                assert (b[at], b[at + 8]) == (hi, lo), (r, k, c)
    # tap 1 is the plain split of the rows; the packed form has no boundaries but its gap rows
    assert np.array_equal(WC.split_taps_t(x, T=T_, valid=valid).reshape(2, 3, C, 32)[:, 1], W.split_rows_t(x, valid).reshape(2, C, 32))
    a3 = WC.tap_columns(np.nan_to_num(x), valid=valid, packed=True)
    assert np.array_equal(a3[4, :C], x[3]) and not a3[8, :C].any() and np.array_equal(a3[8, 2 * C:], x[9]) and not a3[5, 2 * C:].any()


def test_split_entry_refuses_bad_arguments():
    lib = _native.load_library()
    assert "hificar_debug_split_taps_t" in _native.SYMBOLS
    x, out, n = np.zeros((8, 128), dtype=np.float32), np.zeros(3 * 128 * 32, dtype=np.uint8), ctypes.c_size_t(0)
    lens = np.array([3, 5], dtype=np.int32)
    call = lambda M, C, T_, l, p, how, xp=x.ctypes.data, op=out.ctypes.data: lib.hificar_debug_split_taps_t(  # noqa: E731
        M, C, T_, l, p, how, xp, op, out.size, ctypes.byref(n))
    assert call(8, 128, 0, None, None, 0) == 0 and call(8, 128, 4, lens.ctypes.data, None, 0) == 0
    for bad in (call(0, 128, 0, None, None, 0), call(8, 0, 0, None, None, 0), call(8, 128, 0, None, None, 2), call(8, 128, 0, None, None, 0, xp=None),
                call(8, 128, 0, None, None, 0, op=None), call(8, 128, 3, lens.ctypes.data, None, 0), call(8, 128, 3, None, None, 0),
                call(8, 128, -1, None, None, 0), call(8, 128, 0, lens.ctypes.data, None, 0), call(8, 128, 4, lens.ctypes.data, lens.ctypes.data, 0)):
        assert bad == E_INVALID
    small = np.zeros(8, dtype=np.uint8)
    assert lib.hificar_debug_split_taps_t(8, 128, 0, None, None, 0, x.ctypes.data, small.ctypes.data, small.size, ctypes.byref(n)) == E_INVALID
    assert n.value == 3 * 128 * 32 and not small.any()


# ------------------------------------------------------------------------------------------------ the emulation and its bars
@pytest.fixture(scope="module")
def emulated():
    return EC.emulated_errors(verbose=True)


def test_recorded_bars_follow_the_rule():
    for k, e in EC.EMULATED.items():
        want = E.X3_OUT_BAR if k == "out" else (EA.BARS_X3WA[k] if e <= EA.BARS_X3WA[k] / 4 else 4 * e)
        assert EC.BARS_X3WAC[k] == want, k
    assert set(EC.EMULATED) == set(EA.EMULATED) == set(EC.BARS_X3WAC)
    assert 0 < EC.EMULATED["out"] < 1e-4 and EC.BARS_X3WAC["out"] == 2e-4 < E.NORTH_STAR_TOL
    assert all(EC.BARS_X3WAC[k] >= EA.BARS_X3WA[k] for k in EC.BARS_X3WAC)  # never tighter than the arithmetic it extends
    assert set(EC.CASES) <= set(O.SHAPES) and set(EC.EDGE_CASES) <= set(O.EDGE_SHAPES) and set(EC.RAGGED_CASES) <= set(R.RAGGED_SHAPES)
    assert set(EC.EXTRA_CASES) <= set(WC.EXTRA_SHAPES)
    assert set(EC.CASES + EC.EDGE_CASES + EC.EXTRA_CASES) == set(WC.DENSE_CASES) and EC.RAGGED_CASES == WC.RAGGED_CASES  # the GPU cases, all of them


def test_emulated_errors_are_below_a_quarter_of_the_bars(emulated):
    worst, gap = emulated
    assert set(worst) == set(EC.BARS_X3WAC)
    for k, e in sorted(worst.items()):
        print(f"  {k}: emulated {e:.3g}, recorded {EC.EMULATED[k]:g}, device bar {EC.BARS_X3WAC[k]:g}")
        assert 0 < e <= EC.EMULATED[k] and e <= EC.BARS_X3WAC[k] / 4, k
    assert gap < E.X3_OUT_BAR  # the forward is bf16x3wa's: the ReLU-side condition holds as it does there


@pytest.mark.parametrize("name", ["t65", "nores"])
def test_the_emulation_reroutes_the_selected_convs_gradients_and_nothing_else(name):
    """Against the bf16x3wa emulation on the same case: out, loss, dx, statistics, running buffers and every other gradient are equal to the
    bit; the weight and bias gradients of the selected convs move, and stay within a quarter of the gradient bar of float64."""
    with EA.emulating():
        a = O.restatement(name, torch.float64)
    with EC.emulating():
        b = O.restatement(name, torch.float64)
    assert O.banded_attention_train is EA._attention and O.F is torch.nn.functional and E.linear3 is EW._linear3  # (the reroutes are undone)
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["dx"], b["dx"]) and torch.equal(a["stats"], b["stats"]) and float(a["loss"]) == float(b["loss"])
    assert all(torch.equal(a["running"][k], v) for k, v in b["running"].items())
    moved = {k for k in a["grads"] if not torch.equal(a["grads"][k], b["grads"][k])}
    params = O.SHAPES[name][0]
    assert moved == set(WC.moved_tensors(params)) and len(moved) == (12 if name == "nores" else 10)
    ref = O.restatement(name, torch.float64, gates=b["sides"])
    for k in moved:
        assert float((b["grads"][k] - ref["grads"][k]).abs().max()) / O.grad_scale(ref["grads"], k) < EC.BARS_X3WAC["grad"] / 4, k


# ------------------------------------------------------------------------------------------------ the rule and what the GPU cases reach
def test_the_rule_selects_the_layers_the_issue_names():
    names = lambda p: [L.name for L in W.layers(p) if WC.gemm3_form(L)]  # noqa: E731
    five = ["conv_blocks.2.conv2", "conv_blocks.2.conv1", "conv_blocks.1.conv2", "conv_blocks.1.conv1", "conv_blocks.0.conv2"]
    for hidden in (128, 768, 1024):
        assert names(dict(in_channels=12, out_channels=80, elayers=1, hidden_dim=hidden)) == five
    assert names(dict(in_channels=128, out_channels=8, elayers=1, hidden_dim=128)) == five + ["conv_blocks.0.conv1"]      # nores
    assert names(dict(in_channels=97, out_channels=8, elayers=1, hidden_dim=256)) == five + ["conv_blocks.0.conv1"]       # pads to 128
    assert names(dict(in_channels=1024, out_channels=8, elayers=1, hidden_dim=256)) == five + ["conv_blocks.0.conv1"]
    assert names(dict(in_channels=96, out_channels=8, elayers=1, hidden_dim=256)) == five                                 # narrow
    assert names(dict(in_channels=1025, out_channels=8, elayers=1, hidden_dim=256)) == five                               # 3 x 1056 > 3072
    # residual_path and w_out have one tap; no one-tap layer is selected twice
    assert not any(WC.gemm3_form(L) and W.gemm_form(L) for L in W.layers(dict(in_channels=200, out_channels=200, elayers=1, hidden_dim=256)))
    assert not WC.gemm3_form(W.Layer("a", 96, 128, 3, True)) and WC.gemm3_form(W.Layer("a", 97, 128, 3, True))
    for cout, cin, K in ((768, 768, 3), (768, 768, 1), (768, 12, 3), (128, 128, 3), (128, 1024, 3), (128, 1025, 3), (96, 128, 3), (128, 97, 3), (128, 96, 3)):
        assert EC.gemm3_form(cout, cin, K) == WC.gemm3_form(W.Layer("a", cout, cin, K, True)), (cout, cin, K)


def all_launches():
    runs = [(name, "dense") for name in WC.DENSE_CASES] + [(name, form) for name in WC.RAGGED_CASES for form in ("ragged", "packed")]
    return {run: WC.case_launches(*run) for run in runs}


def test_the_gpu_cases_reach_every_path_of_the_launch():
    runs = all_launches()
    every = [l for moved, _, _ in runs.values() for l in moved]
    assert all(len(moved) in (5, 6) and onetap and rest for moved, onetap, rest in runs.values())  # w_out stays in fp32 in every case
    assert all((l.aj, l.rchunk) == (4, 32) and l.tiles_a >= 2 for l in every)                      # at least 12 column blocks: the wide tile, more than one
    six = ("nores", "pad101")                                                                      # conv_blocks.0.conv1 moves too
    assert {len(m) for (name, _), (m, _, _) in runs.items() if name in six} == {6} and {len(m) for (name, _), (m, _, _) in runs.items() if name not in six} == {5}
    assert any(l.layer.cin != WC.pad32(l.layer.cin) and l.layer.cin % 4 for l in every)            # pad101: the taps' pitch is not the gradient's, rows on no 16-byte boundary
    assert any(l.rows < 8 for l in every)                                                          # t2: one partial group, every frame a first or a last
    assert any(l.rows % 8 for l in every) and any(l.rows % 8 == 0 for l in every)
    T65 = WC.case_shape("t65")[2]
    assert T65 % 8 == 1                                                                            # t65: a sequence boundary inside a group
    cols = {3 * WC.pad32(l.layer.cin) for l in every}
    assert {384, 1152, 3072} <= cols                                                               # nores / hidden 128; d48; rows4112 fills the buffer
    assert any(3 * WC.pad32(l.layer.cin) % 256 for l in every)                                     # 384: the second 256-column tile half empty
    assert any(-(-l.nchunks // l.nsplit) >= 3 for l in every if 3 * WC.pad32(l.layer.cin) == 3072)  # rows4112: a split owns several chunks
    assert any(l.nsplit == 1 for l in every) and any(l.nsplit > 1 for l in every) and any(l.nchunks % l.nsplit for l in every)
    assert any(l.tiles_g == 1 for l in every) and any(l.tiles_g > 1 for l in every)
    assert all(1 <= l.nsplit <= l.nchunks for l in every)                                          # every split owns a chunk
    assert all(l.layer.bias for l in every)
    for name in WC.RAGGED_CASES:
        assert WC.case_rows(name, "packed") != WC.case_rows(name, "ragged")


def test_expected_rows_carry_the_convs_own_shape():
    moved, onetap, rest = WC.case_launches("d48")
    rows = WC.expected_rows(moved)
    assert list(rows) == [("wgrad_bf16x3_kernel<4,32> 384x384k3p1", "r1 n1")] and rows[("wgrad_bf16x3_kernel<4,32> 384x384k3p1", "r1 n1")][0] == 5
    assert not set(rows) & set(W.expected_rows(onetap))                                            # the one-tap rows say k1
    assert [(L.name, L.K) for L in rest] == [("w_out", 1), ("conv_blocks.0.conv1", 3), ("conv_blocks.0.residual_path", 1)]
    assert W.parse_row("wgrad_bf16x3_kernel<4,32> 384x384k3p1 s7 r1 n1") == ("wgrad_bf16x3_kernel<4,32>", (384, 384, 3), 7,
                                                                           ("wgrad_bf16x3_kernel<4,32> 384x384k3p1", "r1 n1"))
    # the twin's split, not the taps form's: 3 x 5 tiles of 128 x 256 over 260 rows
    assert moved[0].nsplit == W.wgrad_split(WC.twin(moved[0].layer), 260) and (moved[0].tiles_g, moved[0].tiles_a) == (3, 5)


# ------------------------------------------------------------------------------------------------ the Python surface and the C ABI
def test_keyword_setter_copies_and_refusals():
    assert _native.PREC_BF16X3WAC == 6 and _native.XFMR_TRAIN_PRECISIONS_ALL == dict(_native.XFMR_TRAIN_PRECISIONS, bf16x3wac=6)
    assert _native.TRAIN_PRECISIONS == {"f32": 0, "bf16x3": 1, "bf16x3w": 2} and _native.XFMR_TRAIN_PRECISIONS == dict(_native.TRAIN_PRECISIONS, bf16x3wa=4)
    assert "bf16x3wac" not in _native.XFMR_PRECISIONS
    m = Transformer(train_precision="bf16x3wac", **O.BASE)
    assert m.train_precision == "bf16x3wac" and m.precision == "f32"
    assert copy.deepcopy(m).train_precision == "bf16x3wac" and pickle.loads(pickle.dumps(m)).train_precision == "bf16x3wac"
    assert not any("precision" in k for k in m.state_dict())
    for to in ("bf16x3wa", "bf16x3w", "bf16x3", "f32", "bf16x3wac"):  # (no handle yet: the choice alone)
        m.set_train_precision(to)
        assert m.train_precision == to
    # the inference arithmetic does not know the value
    with pytest.raises(ValueError, match="precision must be one of"):
        Transformer(precision="bf16x3wac", **O.BASE)
    with pytest.raises(ValueError, match="precision must be one of"):
        Transformer(**O.BASE).set_precision("bf16x3wac")
    for inference in ("bf16x3", "bf16x3a"):
        with pytest.raises(ValueError, match="inference-only"):
            Transformer(precision=inference, train_precision="bf16x3wac", **O.BASE)
        with pytest.raises(ValueError, match="inference-only"):
            Transformer(precision=inference, **O.BASE).set_train_precision("bf16x3wac")
        with pytest.raises(ValueError, match="inference-only"):
            m.set_precision(inference)
    for bad in ("bf16x3WAC", "bf16x3wc", "bf16x3ac", 6):
        with pytest.raises(ValueError, match="train_precision must be one of"):
            Transformer(train_precision=bad, **O.BASE)
        with pytest.raises(ValueError, match="train_precision must be one of"):
            Transformer(**O.BASE).set_train_precision(bad)
    with pytest.raises(NotImplementedError, match="on the device only"):
        Transformer(train_precision="bf16x3wac", **O.BASE).train()(torch.zeros(2, 12, 5))


def test_the_trainer_reads_the_config_key(caplog):
    cpu = torch.device("cpu")
    with caplog.at_level(logging.INFO):
        tr = T.InversionTrainer(config(train_precision="bf16x3wac"), cpu)
    assert tr.G.train_precision == "bf16x3wac" and tr.G.precision == "f32" and tr.train_precision == "bf16x3wac"
    assert "training arithmetic bf16x3wac" in caplog.records[0].getMessage()
    bigru = dict(config(), generator_type="BiGRU", generator_params=dict(in_channels=12, out_channels=8))
    with pytest.raises(NotImplementedError, match="train_precision bf16x3wac is built for generator_type Transformer"):
        T.InversionTrainer(dict(bigru, train_precision="bf16x3wac"), cpu)
    with pytest.raises(ValueError, match="train_precision must be"):
        T.InversionTrainer(config(train_precision="bf16x3wc"), cpu)
    assert set(tr.G.state_dict()) == set(T.InversionTrainer(config(), cpu).G.state_dict())  # a checkpoint does not know the arithmetic


def test_only_the_training_switch_takes_the_value():
    lib = _native.load_library()
    h = ctypes.c_void_p()
    cfg = _native.make_xfmr_config(O.BASE)
    _native.check(lib.hificar_xfmr_create(ctypes.byref(cfg), ctypes.byref(h)), "hificar_xfmr_create")
    WAC = _native.PREC_BF16X3WAC
    try:
        # to and from every other training arithmetic
        for p in (WAC, _native.PREC_BF16X3WA, WAC, _native.PREC_BF16X3W, WAC, _native.PREC_BF16X3, WAC, _native.PREC_F32, WAC, WAC):
            assert lib.hificar_xfmr_set_train_precision(h, p) == 0
        for bad in (3, 5, 7, -1):
            assert lib.hificar_xfmr_set_train_precision(h, bad) == E_INVALID and b"precision" in lib.hificar_last_error()
        assert lib.hificar_xfmr_set_precision(h, WAC) == E_INVALID and b"unknown precision 6" in lib.hificar_last_error()
        assert lib.hificar_xfmr_set_train_precision(h, _native.PREC_F32) == 0
        assert lib.hificar_xfmr_set_precision(h, _native.PREC_BF16X3) == 0  # an inference handle has no training arithmetic, this one neither
        assert lib.hificar_xfmr_set_train_precision(h, WAC) == E_STATE and b"inference" in lib.hificar_last_error()
    finally:
        lib.hificar_xfmr_destroy(h)
    # the generator's config and switch (the conv engine's arithmetic)
    p = dict(E2W_PARAMS, use_tanh=True)
    bad = _native.make_config(p, WAC)
    assert lib.hificar_create(ctypes.byref(bad), ctypes.byref(h)) == E_INVALID and b"unknown precision 6" in lib.hificar_last_error()
    ok = _native.make_config(p, _native.PREC_F32)
    _native.check(lib.hificar_create(ctypes.byref(ok), ctypes.byref(h)), "hificar_create")
    try:
        assert lib.hificar_set_precision(h, WAC) == E_INVALID and b"unknown precision 6" in lib.hificar_last_error()
    finally:
        lib.hificar_destroy(h)
    header = open(os.path.join(REPO, "include", "hificar.h")).read()
    assert "#define HIFICAR_PREC_BF16X3WAC 6 " in header
    assert "bf16x3 weight gradients of the k = 3 convs" not in header
