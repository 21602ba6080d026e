"""The Transformer's opt-in bf16x3w training arithmetic on a MI355X (``train_precision="bf16x3w"``: the bf16x3 step, and the weight and bias
gradients of the one-tap GEMM-form layers — w_raw_in, q | k | v, w_o, linear1, linear2 — in wgrad_bf16x3_kernel on rows
xfmr_split_rows_t_kernel splits).  ``pytest -m gpu``.

Per case (tests/transformer_bf16x3w_forms.py: DENSE_CASES, and the ragged batch padded and packed): the profile rows by name, both ways; every
quantity against the float64 restatement on the device's own ReLU sides, within transformer_train_bf16x3w_emulation.BARS_X3W — set on the
CPU before the first GPU run, tests/test_transformer_train_bf16x3w_host.py holds the emulation to a quarter of them; a ReLU may be taken on
another side than float64 takes it only where float64's input lies within the bf16x3 output bar (2e-4, relative) of zero; everything but the
GEMM-form tensors' gradients bitwise a bf16x3 step's; repeats on dirty scratch; the switches back.
"""

import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import transformer_bf16x3w_forms as W
import transformer_ragged_oracle as R
import transformer_train_bf16x3_emulation as E
import transformer_train_bf16x3w_emulation as EW
import transformer_train_oracle as O
from test_gpu_transformer_packed import native_packed_step, pstep
from test_gpu_transformer_ragged import native_step, padded
from test_gpu_transformer_train import assert_within, batch_of, dev, step, steps_config
from test_transformer_train_bf16x3w_host import gemm_form_tensors, split_cases
from articulatory_amd import _native
from articulatory_amd.bin.train import InversionTrainer
from articulatory_amd.models import Transformer
from articulatory_amd.models.transformer import _grad_layout
from articulatory_amd.utils.synth import uniform

pytestmark = pytest.mark.gpu

REFERENCE_ON_THE_DEVICE = ("rows4112",)  # as tests/test_gpu_transformer_train_edges.py, which holds that float64 run to the host's
_CASES, _RUNS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def detail_env():
    """HIFICAR_PROFILE_DETAIL=1: weight-gradient rows carry the instantiation and the layer's shape.  Read when a native handle is built."""
    mp = pytest.MonkeyPatch()
    mp.setenv("HIFICAR_PROFILE_DETAIL", "1")
    yield mp
    mp.undo()


def case(name):
    """(params with dropout, state_dict, x, t, shapes) of a dense case, drawn once."""
    if name not in _CASES:
        shapes = O.EDGE_SHAPES if name in O.EDGE_SHAPES else None
        _CASES[name] = O.case(name, shapes=shapes) + (shapes,)
    return _CASES[name]


def model(params, sd, arithmetic, offset=0):
    m = Transformer(train_precision=arithmetic, **params)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to("cuda:0").train()
    m.set_dropout_seed(O.DROPOUT_SEED, offset=offset)
    return m


def profiled(m, fn):
    """(fn's result, {profile row: launches} of what it launched on the model's engine)."""
    eng = m.engine()  # (first: it is what loads m._lib)
    lib = m._lib
    _native.check(lib.hificar_profile_begin(eng), "hificar_profile_begin")
    out = fn()
    rows, n = _native.profile_rows(lib, eng, 512)
    assert n < 512
    return out, {r["name"]: r["launches"] for r in rows}


def check_rows(name, form, rows_w, rows_3):
    """The profile of a bf16x3w step (rows_w) by name, both ways, against the restated rule and against the bf16x3 step's (rows_3)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    launches, rest = W.case_launches(name, form, num_cus=cus)
    assert launches and rest
    new = {r: n for r, n in rows_w.items() if r.startswith("wgrad_bf16x3_kernel")}
    got = {}
    for r, n in new.items():
        _, _, s, key = W.parse_row(r)
        assert key not in got, r
        got[key] = (n, s)
    assert got == W.expected_rows(launches), (name, form, got, W.expected_rows(launches))       # exactly the GEMM-form layers, each instantiation and split
    assert not any(r.startswith("wgrad_gemm_kernel") for r in rows_w)                               # ... and none of them in fp32
    assert rows_w.get("xfmr_split_rows_t_kernel", 0) == 2 * len(launches)                           # G and A of every such launch
    other = {r: n for r, n in rows_w.items() if r.startswith("wgrad_") and r not in new}
    shapes = collections.Counter()
    for r, n in other.items():
        shapes[W.parse_row(r)[1]] += n
    assert shapes == collections.Counter((L.cout, L.cin, L.K) for L in rest), (name, form, other)   # fp32 rows for the rest, all of it
    # the bf16x3 step: the same layers in wgrad_gemm_kernel with the same splits, no new kernel, and every other weight-gradient row,
    # every reduction and everything else the same launches
    assert not any(r.startswith(("wgrad_bf16x3_kernel", "xfmr_split_rows_t_kernel")) for r in rows_3)
    gemm = {}
    for r, n in rows_3.items():
        if r.startswith("wgrad_gemm_kernel"):
            kernel, shape, s, _ = W.parse_row(r)
            gemm[(kernel.replace("wgrad_gemm_kernel", "wgrad_bf16x3_kernel") + " " + r.split(" ")[1], "r1 n1")] = (n, s)
    assert gemm == got, (name, form, gemm, got)
    drop = ("wgrad_bf16x3_kernel", "wgrad_gemm_kernel", "xfmr_split_rows_t_kernel")
    assert {r: n for r, n in rows_w.items() if not r.startswith(drop)} == {r: n for r, n in rows_3.items() if not r.startswith(drop)}
    assert any(r.startswith("wreduce_kernel") for r in rows_w) and any(r.startswith("conv_bf16x3") for r in rows_w)


def assert_same_but_the_gemm_form_gradients(a, b, params, what):
    """Two steps in the restatement's layout: everything bitwise equal but the gradients bf16x3w computes on bf16 MFMAs, which differ."""
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["loss"], b["loss"]) and torch.equal(a["dx"], b["dx"]) and torch.equal(a["stats"], b["stats"]), what
    assert all(torch.equal(a["running"][k], v) for k, v in b["running"].items()), what
    moved = set(gemm_form_tensors(params))
    assert moved <= set(a["grads"]) == set(b["grads"])
    for k, g in b["grads"].items():
        assert torch.isfinite(a["grads"][k]).all() and torch.equal(a["grads"][k], g) == (k not in moved), (what, k)


def assert_equal_steps(a, b, what):
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["dx"], b["dx"]) and torch.equal(a["stats"], b["stats"]), what
    assert set(a["grads"]) == set(b["grads"]) and all(torch.equal(a["grads"][k], g) for k, g in b["grads"].items()), what


def same(a, b, m, what):
    """(out, statistics, gradient buffer, dx) of two runs of the C entry points, bit for bit and finite."""
    for q, u, v in zip(("out", "batch statistics", None, "dx"), a, b):
        if q is not None:
            assert torch.isfinite(v).all() and torch.equal(u, v), (what, q)
    for key, off, num in _grad_layout(m):
        assert torch.isfinite(b[2][off:off + num]).all() and torch.equal(a[2][off:off + num], b[2][off:off + num]), (what, key)


def run(name):
    """One bf16x3w step of a dense case with its profile, the float64 reference on its ReLU sides, and the bf16x3 step of the same model and
    seed with its profile: computed once per module and left unchanged."""
    if name not in _RUNS:
        params, sd, x, t, shapes = case(name)
        mw = model(params, sd, "bf16x3w")
        gates = {}
        got = step(mw, x, t, gates=gates)
        ref = O.restatement(name, torch.float64, device="cuda:0" if name in REFERENCE_ON_THE_DEVICE else "cpu", gates=gates, shapes=shapes)
        mw2 = model(params, sd, "bf16x3w")
        again, rows_w = profiled(mw2, lambda: step(mw2, x, t))
        m3 = model(params, sd, "bf16x3")
        x3, rows_3 = profiled(m3, lambda: step(m3, x, t))
        _RUNS[name] = dict(got=got, ref=ref, again=again, rows_w=rows_w, x3=x3, rows_3=rows_3, model=mw)
    return _RUNS[name]


# ------------------------------------------------------------------------------------------------ the dense cases
@pytest.mark.parametrize("name", W.DENSE_CASES)
def test_profile_rows_by_name_both_ways(name):
    r = run(name)
    print("  " + "\n  ".join(sorted(k for k in r["rows_w"] if k.startswith(("wgrad_", "xfmr_split_rows_t")))))
    check_rows(name, "dense", r["rows_w"], r["rows_3"])


@pytest.mark.parametrize("name", W.DENSE_CASES)
def test_step_against_the_restatement(name):
    r = run(name)
    got, ref = r["got"], r["ref"]
    print(f"  {name}: {ref['gate_flips']} ReLU(s) on the other side than float64's own, the farthest {ref['gate_gap']:.3g} of max |x| from zero")
    assert ref["gate_gap"] < E.X3_OUT_BAR
    assert set(got["grads"]) == set(ref["grads"])
    errs = EW.errors_x3w(got, ref)
    moved = ["grad." + k for k in gemm_form_tensors(case(name)[0])]
    print("  the GEMM-form tensors' worst: %s" % ", ".join(f"{k} {errs[k][0]:.3g}" for k in sorted(moved, key=lambda k: -errs[k][0])[:3]))
    assert_within(errs, name)
    assert torch.isfinite(got["out"]).all() and torch.isfinite(got["dx"]).all()
    assert "libhificar.so" in open("/proc/self/maps").read()


@pytest.mark.parametrize("name", W.DENSE_CASES)
def test_everything_else_is_bitwise_the_bf16x3_step_and_repeats_are_bit_identical(name):
    r = run(name)
    params = case(name)[0]
    assert_same_but_the_gemm_form_gradients(r["got"], r["x3"], params, name)
    assert_equal_steps(r["got"], r["again"], name + " on a second model")  # (with and without the debug taps)
    # the moved gradients differ from the fp32 kernels' by rounding, not by more: both lie within the bar of float64, so within two of each other
    for k in gemm_form_tensors(params):
        d = float((r["got"]["grads"][k] - r["x3"]["grads"][k]).abs().max()) / O.grad_scale(r["ref"]["grads"], k)
        assert 0 < d < 2 * EW.BARS_X3W["grad"], (name, k, d)


@pytest.mark.parametrize("name", W.DENSE_CASES)
def test_dirty_scratch_equal_lengths_and_the_switches_back(name):
    params, sd, x, t, _ = case(name)
    B, _, T = x.shape
    p, seed = params["dropout"], O.SEEDS[name]
    m = model(params, sd, "bf16x3w")
    m._native_handle(train=True)
    xd = dev(x)
    dout = dev(uniform(seed, "dout", (B, params["out_channels"], T), -1.0, 1.0))
    # what tape, workspace and outputs hold on entry does not matter; every length = T through the ragged entry is the dense step
    dense = native_step(m, xd, dout, p, 0x00)
    same(dense, native_step(m, xd, dout, p, 0xFF), m, "0xFF-filled buffers")
    same(dense, native_step(m, xd, dout, p, 0xFF, lengths=[T] * B), m, "every length = T")
    assert float(dense[3].abs().max()) > 0
    # forward_padded with every length = T: the dense autograd step
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m.set_dropout_seed(O.DROPOUT_SEED)
    m.zero_grad(set_to_none=True)
    xt = xd.clone().requires_grad_(True)
    y = m.forward_padded(xt, [T] * B)
    F.l1_loss(y, dev(t)).backward()  # (the dense step's loss: the same output gradient)
    want = run(name)["got"]
    assert torch.equal(y, want["out"]) and torch.equal(xt.grad, want["dx"]) and torch.equal(m._last_stats, want["stats"])
    assert all(torch.equal(q.grad, want["grads"][k]) for k, q in m.named_parameters())
    # the same handle switched to bf16x3, then to f32: the next steps are those of fresh models in those arithmetics, bitwise
    for arithmetic in ("bf16x3", "f32"):
        m.set_train_precision(arithmetic)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)  # (the running statistics moved)
        m.set_dropout_seed(O.DROPOUT_SEED)
        fresh = run(name)["x3"] if arithmetic == "bf16x3" else step(model(params, sd, "f32"), x, t)
        assert_equal_steps(step(m, x, t), fresh, f"{name} after set_train_precision({arithmetic})")


def test_a_backward_after_a_switch_is_refused_and_the_tape_survives():
    name = "t65"
    params, sd, x, t, _ = case(name)
    straight = run(name)["got"]
    m = model(params, sd, "bf16x3w")
    xt = dev(x).requires_grad_(True)
    loss = F.l1_loss(m(xt), dev(t))
    for other in ("bf16x3", "f32"):
        m.set_train_precision(other)
        with pytest.raises(RuntimeError, match=f"training arithmetic is {other}, its last training forward ran in bf16x3w"):
            loss.backward(retain_graph=True)
        assert xt.grad is None and all(q.grad is None for q in m.parameters())
    m.set_train_precision("bf16x3w")
    loss.backward()
    assert torch.equal(xt.grad, straight["dx"]) and all(torch.equal(q.grad, straight["grads"][k]) for k, q in m.named_parameters())
    # ... and the other way round: a bf16x3 tape does not go back through bf16x3w
    m3 = model(params, sd, "bf16x3")
    loss = F.l1_loss(m3(dev(x)), dev(t))
    m3.set_train_precision("bf16x3w")
    with pytest.raises(RuntimeError, match="training arithmetic is bf16x3w, its last training forward ran in bf16x3"):
        loss.backward()


def test_workspace_grows_by_the_two_split_buffers_behind_the_bf16x3_one():
    params, sd, _, _, _ = case("t65")
    m = model(params, sd, "f32")
    m._native_handle(train=True)
    lib, h = m._lib, m._handle
    host = torch.tensor([70, 33, 1], dtype=torch.int32)
    mp = lib.hificar_xfmr_packed_rows(3, 70, host.data_ptr())
    sizes = lambda: (lib.hificar_xfmr_train_workspace_bytes(h, 2, 65), lib.hificar_xfmr_train_workspace_bytes_packed(h, 3, mp))  # noqa: E731
    tapes = lambda: (lib.hificar_xfmr_tape_bytes(h, 2, 65), lib.hificar_xfmr_tape_bytes_packed(h, 3, mp))  # noqa: E731
    f32, tape = sizes(), tapes()
    m.set_train_precision("bf16x3")
    x3 = sizes()
    m.set_train_precision("bf16x3w")
    x3w = sizes()
    # two buffers of ceil(rows / 8) groups x 3072 columns x 32 bytes (rows: B T + 64 rounded up to 256, or the packed rows), behind bf16x3's one
    assert (x3w[0] - x3[0], x3w[1] - x3[1]) == (2 * 256 * 3072 * 4, 2 * mp * 3072 * 4) and x3[0] - f32[0] == 256 * 3072 * 4
    assert tapes() == tape
    m.set_train_precision("f32")
    assert sizes() == f32


# ------------------------------------------------------------------------------------------------ the ragged batch, padded and packed
def ragged_model(arithmetic):
    params, sd, x, t, lengths = R.ragged_case(W.RAGGED_CASE)
    return model(params, sd, arithmetic), params, x, t, lengths


@pytest.mark.parametrize("form", ["ragged", "packed"])
def test_ragged_and_packed_steps(form):
    m, params, x, t, lengths = ragged_model("bf16x3w")
    gates = {}
    got = pstep(m, x, t, lengths, form=form, gates=gates)
    ref = R.ragged_restatement(W.RAGGED_CASE, torch.float64, gates=gates)
    print(f"  {form}: {ref['gate_flips']} ReLU(s) on the other side than float64's own, the farthest {ref['gate_gap']:.3g} of max |x| from zero")
    assert ref["gate_gap"] < E.X3_OUT_BAR
    assert_within(EW.errors_x3w(got, ref), form)
    assert float(padded(got["out"], lengths).abs().max()) == 0.0 and float(padded(got["dx"], lengths).abs().max()) == 0.0
    mw, m3 = ragged_model("bf16x3w")[0], ragged_model("bf16x3")[0]
    again, rows_w = profiled(mw, lambda: pstep(mw, x, t, lengths, form=form))
    x3, rows_3 = profiled(m3, lambda: pstep(m3, x, t, lengths, form=form))
    check_rows(W.RAGGED_CASE, form, rows_w, rows_3)
    assert_equal_steps(got, again, form + " on a second model")
    assert_same_but_the_gemm_form_gradients(got, x3, params, form)


def test_ragged_and_packed_forms_padded_frames_and_dirty_scratch():
    m, params, x, _, lengths = ragged_model("bf16x3w")
    m._native_handle(train=True)
    B, _, T = x.shape
    p, seed = params["dropout"], R.RAGGED_SEEDS[W.RAGGED_CASE]
    x = dev(x)
    dout = dev(uniform(seed, "dout", (B, params["out_channels"], T), -1.0, 1.0))
    dense = native_step(m, x, dout, p, 0x00)
    # zeros on padded frames; NaN there in x and dout, on 0xFF-filled buffers, changes nothing: the split pass writes such rows as zero
    # bits without reading them
    pad = (~R.valid_mask(lengths, T)).to("cuda:0")[:, None, :]
    xz, dz = x.masked_fill(pad, 0.0).contiguous(), dout.masked_fill(pad, 0.0).contiguous()
    xn, dn = x.masked_fill(pad, float("nan")).contiguous(), dout.masked_fill(pad, float("nan")).contiguous()
    for what, fn in (("ragged", lambda *a: native_step(m, *a, lengths=lengths)), ("packed", lambda *a: native_packed_step(m, *a, lengths))):
        clean, dirty = fn(xz, dz, p, 0x00), fn(xn, dn, p, 0xFF)
        same(clean, dirty, m, what)
        assert float(padded(dirty[0], lengths).abs().max()) == 0.0 and float(padded(dirty[3], lengths).abs().max()) == 0.0, what
        assert not torch.equal(clean[0], dense[0])


# ------------------------------------------------------------------------------------------------ five steps through the trainer
def test_five_steps_through_the_trainer_then_back_to_bf16x3():
    params, sd, _, _ = O.case(O.STEPS_CASE)
    tr = InversionTrainer(dict(steps_config(params), train_precision="bf16x3w"), torch.device("cuda:0"))
    tr.G.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    tr.G.set_dropout_seed(O.DROPOUT_SEED)
    assert tr.G.train_precision == "bf16x3w" and tr.optimizer["generator"].defaults.get("fused") is True
    losses = [float(tr.train_step(batch_of(s))["train/generator_loss"]) for s in range(O.STEPS["n"])]
    ref_losses, ref_final = O.five_steps(torch.float64)
    e_loss, worst = O.five_step_errors(losses, dict(tr.G.state_dict()), ref_losses, ref_final)
    print("losses", losses, "deviation", e_loss, "worst final tensor", max(worst, key=worst.get), max(worst.values()))
    assert e_loss < EW.BARS_X3W["steps_loss"]
    assert max(worst.values()) < EW.BARS_X3W["steps_params"]
    # back to bf16x3 on the same handle: the next step is a fresh bf16x3 model's on the same state_dict, bitwise
    tr.G.set_train_precision("bf16x3")
    fresh = Transformer(train_precision="bf16x3", **params)
    fresh.load_state_dict(tr.G.state_dict(), strict=True)
    fresh = fresh.to("cuda:0").train()
    fresh.set_dropout_seed(O.DROPOUT_SEED, offset=tr.G._calls)
    _, _, x, t = O.case(O.STEPS_CASE, 7)
    assert_equal_steps(step(tr.G, x, t), step(fresh, x, t), "after five bf16x3w steps")


# ------------------------------------------------------------------------------------------------ the split pass on the device
def test_device_split_bytes_are_the_numpy_restatement():
    """xfmr_split_rows_t_kernel over a buffer of 0xFF bytes against the layout's numpy restatement, byte for byte: rows 1, 7, 8, 9 and 257,
    widths 128, 384 and 3072, a ragged batch's padded frames and a packed batch's gap rows (NaN there in the input)."""
    seen = 0
    for what, got, want in split_cases(1):
        assert got.shape == want.shape and np.array_equal(got, want), what
        seen += 1
    assert seen == 17
