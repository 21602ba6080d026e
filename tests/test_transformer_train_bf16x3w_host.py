"""The Transformer's opt-in bf16x3w TRAINING arithmetic (bf16x3, and the one-tap GEMM-form weight gradients on bf16 MFMAs too), as far as it
goes without a device: the split pass's layout from the library's host entry against a numpy restatement, the CPU emulation that set the GPU
tests' bars (tests/transformer_train_bf16x3w_emulation.py), the Python surface and the C ABI's refusals, and a proof from the restated
dispatch rule (tests/transformer_bf16x3w_forms.py) that the GPU cases reach every path of wgrad_bf16x3_kernel."""

import copy
import ctypes
import logging
import os
import pickle

import numpy as np
import pytest
import torch

import transformer_bf16x3w_forms as W
import transformer_train_bf16x3_emulation as E
import transformer_train_bf16x3w_emulation as EW
import transformer_train_oracle as O
from conftest import E2W_PARAMS, REPO
from test_transformer_train_host import config
from articulatory_amd import _native
from articulatory_amd.bin import train as T
from articulatory_amd.models import Transformer
from articulatory_amd.utils.synth import uniform

E_INVALID, E_STATE = -1, -2


# ------------------------------------------------------------------------------------------------ the split pass's layout
def library_split(x, how, T=0, lengths=None, pad_row=None):
    """hificar_debug_split_rows_t's bytes (how 0: the device pass's index functions on the host; 1: the device pass)."""
    lib = _native.load_library()
    M, C = x.shape
    x = np.ascontiguousarray(x, dtype=np.float32)
    lens = None if lengths is None else np.asarray(lengths, dtype=np.int32)
    pads = None if pad_row is None else np.asarray(pad_row, dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    n = ctypes.c_size_t(0)
    probe = np.zeros(1, dtype=np.uint8)
    assert lib.hificar_debug_split_rows_t(M, C, T, ptr(lens), ptr(pads), how, x.ctypes.data, probe.ctypes.data, 1, ctypes.byref(n)) == E_INVALID
    assert n.value == (M + 7) // 8 * C * 32
    out = np.full(n.value + 64, 0xA5, dtype=np.uint8)
    _native.check(lib.hificar_debug_split_rows_t(M, C, T, ptr(lens), ptr(pads), how, x.ctypes.data, out.ctypes.data, n.value, ctypes.byref(n)),
                  "hificar_debug_split_rows_t")
    assert (out[n.value:] == 0xA5).all()  # nothing behind the split is written
    return out[:n.value]


def ragged_valid(lengths, T):
    return np.concatenate([np.arange(T) < n for n in lengths])


SPLIT_RAGGED = dict(T=9, lengths=(9, 4, 0, 1))                      # M = 36: a full, a partial, an empty and a one-frame sequence
SPLIT_PACKED = [0, 1, 2, -1, 9, 10, 11, 12, 13, -1, 18, -1, -1]     # M = 13 packed rows: three sequences, a gap behind each, a gap-row tail


def split_cases(how):
    for M in (1, 7, 8, 9, 257):
        for C in (128, 384, 3072):
            x = uniform(9300 + M + C, "split", (M, C), -1.0, 1.0)
            yield f"{M}x{C}", library_split(x, how), W.split_rows_t(x)
    nan = np.float32("nan")
    T_, lengths = SPLIT_RAGGED["T"], SPLIT_RAGGED["lengths"]
    valid = ragged_valid(lengths, T_)
    x = uniform(9301, "split.ragged", (valid.size, 128), -1.0, 1.0)
    x[~valid] = nan  # (rows of padded frames are not read)
    yield "ragged", library_split(x, how, T=T_, lengths=lengths), W.split_rows_t(x, valid)
    valid = np.asarray(SPLIT_PACKED) >= 0
    x = uniform(9302, "split.packed", (valid.size, 384), -1.0, 1.0)
    x[~valid] = nan
    yield "packed", library_split(x, how, pad_row=SPLIT_PACKED), W.split_rows_t(x, valid)


def test_split_layout_on_the_host_is_the_numpy_restatement():
    """xfmr_split_rows_t_kernel's index functions, run on the host over a 0xFF-filled buffer, against the layout's definition:
    [ceil(M / 8)][C][hi 8 | lo 8] bf16, rows past M, padded frames and gap rows zero bits."""
    seen = 0
    for what, got, want in split_cases(0):
        assert got.shape == want.shape and np.array_equal(got, want), what
        seen += 1
    assert seen == 17


def test_split_restatement_is_the_definition_element_by_element():
    """The numpy restatement itself against the scalar definition (row r, channel c -> bytes ((r // 8) C + c) 32 + 2 (r % 8), lo 16 further)."""
    x = uniform(9303, "split.def", (11, 128), -1.0, 1.0)
    x[3, 5], x[10, 127] = 0.0, -0.0
    valid = np.ones(11, dtype=bool)
    valid[4] = False
    b = W.split_rows_t(x, valid).view(np.uint16)
    assert b.size == 2 * 128 * 16
    for r in range(16):
        for c in (0, 5, 31, 127):
            at = ((r // 8) * 128 + c) * 16 + r % 8
            if r >= 11 or not valid[r]:
                assert b[at] == 0 and b[at + 8] == 0
                continue
            hi = W.bf16(x[r:r + 1, c])[0]
            lo = W.bf16(x[r:r + 1, c] - (np.uint32(hi) << 16).view(np.float32))[0]
            assert (b[at], b[at + 8]) == (hi, lo), (r, c)
    # hi + lo carries the value to 2^-16 of it: the split is the engine's
    hi, lo = b.reshape(2, 128, 2, 8)[:, :, 0, :], b.reshape(2, 128, 2, 8)[:, :, 1, :]
    back = ((hi.astype(np.uint32) << 16).view(np.float32) + (lo.astype(np.uint32) << 16).view(np.float32)).transpose(0, 2, 1).reshape(16, 128)[:11]
    assert np.abs(back[valid] - x[valid]).max() <= 2.0 ** -16 * np.abs(x).max()


def test_split_entry_refuses_bad_arguments():
    lib = _native.load_library()
    x, out, n = np.zeros((8, 128), dtype=np.float32), np.zeros(128 * 32, dtype=np.uint8), ctypes.c_size_t(0)
    lens = np.array([3, 5], dtype=np.int32)
    call = lambda M, C, T_, l, p, how, xp=x.ctypes.data, op=out.ctypes.data: lib.hificar_debug_split_rows_t(  # noqa: E731
        M, C, T_, l, p, how, xp, op, out.size, ctypes.byref(n))
    assert call(8, 128, 0, None, None, 0) == 0
    for bad in (call(0, 128, 0, None, None, 0), call(8, 0, 0, None, None, 0), call(8, 128, 0, None, None, 2), call(8, 128, 0, None, None, 0, xp=None),
                call(8, 128, 0, None, None, 0, op=None), call(8, 128, 3, lens.ctypes.data, None, 0), call(8, 128, 4, lens.ctypes.data, lens.ctypes.data, 0)):
        assert bad == E_INVALID


# ------------------------------------------------------------------------------------------------ the emulation and its bars
@pytest.fixture(scope="module")
def emulated():
    return EW.emulated_errors(verbose=True)


def test_recorded_bars_follow_the_rule():
    for k, e in EW.EMULATED.items():
        want = E.X3_OUT_BAR if k == "out" else (E.FP32_BARS[k] if e <= E.FP32_BARS[k] / 4 else 4 * e)
        assert EW.BARS_X3W[k] == want, k
    assert set(EW.EMULATED) == set(E.EMULATED)
    assert EW.EMULATED["out"] < 1e-4 and EW.BARS_X3W["out"] == 2e-4 < E.NORTH_STAR_TOL
    assert set(EW.CASES) <= set(O.SHAPES) and set(EW.EDGE_CASES) <= set(O.EDGE_SHAPES)
    assert set(EW.CASES + EW.EDGE_CASES) == set(W.DENSE_CASES) and EW.RAGGED_CASE == W.RAGGED_CASE  # the GPU cases, all of them


def test_emulated_errors_are_below_a_quarter_of_the_bars(emulated):
    worst, gap = emulated
    assert set(worst) == set(EW.BARS_X3W)
    for k, e in sorted(worst.items()):
        print(f"  {k}: emulated {e:.3g}, recorded {EW.EMULATED[k]:g}, device bar {EW.BARS_X3W[k]:g}")
        assert 0 < e <= EW.EMULATED[k] and e <= EW.BARS_X3W[k] / 4, k
    assert gap < E.X3_OUT_BAR


def test_the_emulation_reroutes_the_gemm_form_gradients_and_nothing_else():
    """Against the bf16x3 emulation on the same case: out, loss, dx, statistics and every other gradient are equal to the bit; the weight and
    bias gradients of w_raw_in, q | k | v, w_o, linear1 and linear2 move, and stay within the gradient bar of float64."""
    name = "t65"
    with E.emulating():
        a = O.restatement(name, torch.float64)
    with EW.emulating():
        b = O.restatement(name, torch.float64)
    assert O.F is torch.nn.functional and E.linear3 is EW._linear3  # (the reroutes are undone)
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["dx"], b["dx"]) and torch.equal(a["stats"], b["stats"]) and float(a["loss"]) == float(b["loss"])
    moved = {k for k in a["grads"] if not torch.equal(a["grads"][k], b["grads"][k])}
    assert moved == set(gemm_form_tensors(O.SHAPES[name][0]))
    ref = O.restatement(name, torch.float64, gates=b["sides"])
    for k in moved:
        assert float((b["grads"][k] - ref["grads"][k]).abs().max()) / O.grad_scale(ref["grads"], k) < EW.BARS_X3W["grad"] / 4, k


def gemm_form_tensors(params):
    """The state_dict names whose gradients the bf16x3w arithmetic computes on bf16 MFMAs (or, the biases, sums from the split rows)."""
    names = []
    for L in W.layers(params):
        if not W.gemm_form(L):
            continue
        if L.name.endswith("qkv"):
            names += [f"transformer.{L.name[:-3]}self_attn.w_{q}" for q in "qkv"]
        elif L.name.endswith("w_o"):
            names.append(f"transformer.{L.name[:-3]}self_attn.w_o")
        else:
            base = L.name if L.name == "w_raw_in" else "transformer." + L.name
            names += [base + ".weight", base + ".bias"]
    return names


# ------------------------------------------------------------------------------------------------ the Python surface and the C ABI
def test_keyword_setter_copies_and_refusals():
    assert set(_native.PRECISIONS) == {"f32", "bf16x3"} and _native.TRAIN_PRECISIONS == dict(_native.PRECISIONS, bf16x3w=2) and _native.PREC_BF16X3W == 2
    m = Transformer(train_precision="bf16x3w", **O.BASE)
    assert m.train_precision == "bf16x3w" and m.precision == "f32"
    assert copy.deepcopy(m).train_precision == "bf16x3w" and pickle.loads(pickle.dumps(m)).train_precision == "bf16x3w"
    assert not any("precision" in k for k in m.state_dict())
    for to in ("bf16x3", "f32", "bf16x3w"):  # (no handle yet: the choice alone)
        m.set_train_precision(to)
        assert m.train_precision == to
    # the inference arithmetic does not know the value
    with pytest.raises(ValueError, match="precision must be one of"):
        Transformer(precision="bf16x3w", **O.BASE)
    with pytest.raises(ValueError, match="precision must be one of"):
        Transformer(**O.BASE).set_precision("bf16x3w")
    with pytest.raises(ValueError, match="inference-only"):
        Transformer(precision="bf16x3", train_precision="bf16x3w", **O.BASE)
    with pytest.raises(ValueError, match="inference-only"):
        Transformer(precision="bf16x3", **O.BASE).set_train_precision("bf16x3w")
    with pytest.raises(ValueError, match="inference-only"):
        m.set_precision("bf16x3")
    for bad in ("bf16x3W", "bf16w", 2):
        with pytest.raises(ValueError, match="train_precision"):
            Transformer(train_precision=bad, **O.BASE)
    with pytest.raises(NotImplementedError, match="on the device only"):
        Transformer(train_precision="bf16x3w", **O.BASE).train()(torch.zeros(2, 12, 5))


def test_the_trainer_reads_the_config_key(caplog):
    cpu = torch.device("cpu")
    with caplog.at_level(logging.INFO):
        tr = T.InversionTrainer(config(train_precision="bf16x3w"), cpu)
    assert tr.G.train_precision == "bf16x3w" and tr.G.precision == "f32" and tr.train_precision == "bf16x3w"
    assert "training arithmetic bf16x3w" in caplog.records[0].getMessage()
    bigru = dict(config(), generator_type="BiGRU", generator_params=dict(in_channels=12, out_channels=8))
    with pytest.raises(NotImplementedError, match="train_precision bf16x3w is built for generator_type Transformer"):
        T.InversionTrainer(dict(bigru, train_precision="bf16x3w"), cpu)
    assert set(tr.G.state_dict()) == set(T.InversionTrainer(config(), cpu).G.state_dict())  # a checkpoint does not know the arithmetic


def test_only_the_training_switch_takes_the_value():
    lib = _native.load_library()
    assert "hificar_debug_split_rows_t" in _native.SYMBOLS
    h = ctypes.c_void_p()
    cfg = _native.make_xfmr_config(O.BASE)
    _native.check(lib.hificar_xfmr_create(ctypes.byref(cfg), ctypes.byref(h)), "hificar_xfmr_create")
    try:
        for p in (_native.PREC_BF16X3W, _native.PREC_BF16X3, _native.PREC_BF16X3W, _native.PREC_F32, _native.PREC_BF16X3W):
            assert lib.hificar_xfmr_set_train_precision(h, p) == 0
        assert lib.hificar_xfmr_set_train_precision(h, 3) == E_INVALID and b"precision" in lib.hificar_last_error()
        assert lib.hificar_xfmr_set_precision(h, _native.PREC_BF16X3W) == E_INVALID and b"unknown precision 2" in lib.hificar_last_error()
        assert lib.hificar_xfmr_set_train_precision(h, _native.PREC_F32) == 0
        assert lib.hificar_xfmr_set_precision(h, _native.PREC_BF16X3) == 0  # an inference handle has no training arithmetic, this one neither
        assert lib.hificar_xfmr_set_train_precision(h, _native.PREC_BF16X3W) == E_STATE and b"inference" in lib.hificar_last_error()
    finally:
        lib.hificar_xfmr_destroy(h)
    # the generator's config and switch (the conv engine's arithmetic)
    p = dict(E2W_PARAMS, use_tanh=True)
    bad = _native.make_config(p, _native.PREC_BF16X3W)
    assert lib.hificar_create(ctypes.byref(bad), ctypes.byref(h)) == E_INVALID and b"unknown precision 2" in lib.hificar_last_error()
    ok = _native.make_config(p, _native.PREC_F32)
    _native.check(lib.hificar_create(ctypes.byref(ok), ctypes.byref(h)), "hificar_create")
    try:
        assert lib.hificar_set_precision(h, _native.PREC_BF16X3W) == E_INVALID and b"unknown precision 2" in lib.hificar_last_error()
    finally:
        lib.hificar_destroy(h)
    assert "#define HIFICAR_PREC_BF16X3W 2 " in open(os.path.join(REPO, "include", "hificar.h")).read()


# ------------------------------------------------------------------------------------------------ what the GPU cases reach
def all_launches():
    runs = [(name, "dense") for name in W.DENSE_CASES] + [(W.RAGGED_CASE, "ragged"), (W.RAGGED_CASE, "packed")]
    return {(name, form): W.case_launches(name, form) for name, form in runs}


def test_the_rule_selects_the_layers_the_issue_names():
    ls = W.layers(dict(in_channels=12, out_channels=80, elayers=1, hidden_dim=768))
    assert [L.name.split(".")[-1] for L in ls if W.gemm_form(L)] == ["linear2", "linear1", "w_o", "qkv", "w_raw_in"]
    assert [L.name.split(".")[-1] for L in ls if not W.gemm_form(L)] == ["w_out", "conv2", "conv1", "conv2", "conv1", "conv2", "conv1", "residual_path"]
    assert W.gemm_form(W.Layer("a", 97, 128, 1, True)) and not W.gemm_form(W.Layer("a", 96, 128, 1, True)) and not W.gemm_form(W.Layer("a", 128, 96, 1, True))
    assert not W.gemm_form(W.Layer("a", 768, 768, 3, True))
    assert EW.gemm_form(768, 768, 1) and not EW.gemm_form(768, 768, 3) and not EW.gemm_form(768, 12, 1) and not EW.gemm_form(80, 768, 1)


def test_the_gpu_cases_reach_every_path_of_the_kernel():
    runs = all_launches()
    every = [l for ls, _ in runs.values() for l in ls]
    assert all(rest for _, rest in runs.values())                                   # a layer per case that must stay on the fp32 kernels
    assert all(ls for ls, _ in runs.values())
    assert any(l.rows < 8 for l in every)                                           # one partial group, nothing else (t2)
    assert any(l.rows % 8 for l in every) and any(l.rows % 8 == 0 for l in every)   # zero rows inside the last group, and none
    assert any(l.rows % l.rchunk for l in every if l.rows > l.rchunk)               # a partial last chunk
    for aj in (2, 4):                                                               # both tile widths, each with ...
        mine = [l for l in every if l.aj == aj]
        assert any(-(-l.nchunks // l.nsplit) >= 3 for l in mine)                    # ... a split owning >= 3 chunks: the two-buffer ring wraps
        assert any(l.nsplit == 1 for l in mine) and any(l.nsplit > 1 for l in mine)
        assert any(l.tiles_g == 1 for l in mine) and any(l.tiles_g > 1 for l in mine)
        assert any(l.tiles_a > 1 for l in mine) == (aj == 4)                        # (fewer than 256 columns are one 128 x 128 tile's)
        assert any(l.nchunks % l.nsplit for l in mine)                              # splits of unequal length
    assert any(l.aj == 4 and l.layer.cin % 256 for l in every)                      # an A width that is no multiple of the wide tile (384)
    assert any(l.layer.cout % 128 == 0 and l.layer.cin == 3072 for l in every) and any(l.layer.cout == 3072 for l in every)
    assert all(1 <= l.nsplit <= l.nchunks for l in every)                           # every split owns a chunk (the fp32 form's split count fits)
    assert any(l.layer.bias for l in every) and any(not l.layer.bias for l in every)
    # the packed rows differ from the padded rows of the same batch
    assert W.case_rows(W.RAGGED_CASE, "packed") == 256 != W.case_rows(W.RAGGED_CASE, "ragged") == 210


def test_expected_rows_name_the_instantiation():
    ls, _ = W.case_launches("d48")
    rows = W.expected_rows(ls)
    assert rows[("wgrad_bf16x3_kernel<4,32> 384x384k1p1", "r1 n1")][0] == 2       # w_raw_in and w_o
    assert ("wgrad_bf16x3_kernel<4,32> 1152x384k1p1", "r1 n1") in rows and ("wgrad_bf16x3_kernel<4,32> 384x3072k1p1", "r1 n1") in rows
    ls, _ = W.case_launches("t65")
    assert ("wgrad_bf16x3_kernel<2,64> 3072x128k1p1", "r1 n1") in W.expected_rows(ls)
    assert W.parse_row("wgrad_bf16x3_kernel<2,64> 3072x128k1p1 s3 r1 n1") == ("wgrad_bf16x3_kernel<2,64>", (3072, 128, 1), 3,
                                                                             ("wgrad_bf16x3_kernel<2,64> 3072x128k1p1", "r1 n1"))
