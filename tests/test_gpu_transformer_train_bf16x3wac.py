"""The Transformer's opt-in bf16x3wac training arithmetic on a MI355X (``train_precision="bf16x3wac"``: the bf16x3wa step, and the weight and bias
gradients of the wide k = 3 convs as one-tap GEMMs in wgrad_bf16x3_kernel on columns xfmr_split_taps_t_kernel shifts and splits).
``pytest -m gpu``.

Per case (tests/transformer_bf16x3wac_forms.py: DENSE_CASES — the issue's six and pad101, where cin_pad != cin — and the RAGGED_CASES padded and packed): the profile rows by name, both ways,
against the restated rule and against a bf16x3wa step's; every quantity against the float64 restatement on the device's own ReLU sides, within
transformer_train_bf16x3wac_emulation.BARS_X3WAC — set on the CPU before the first GPU run, tests/test_transformer_train_bf16x3wac_host.py
holds the emulation to a quarter of them; a ReLU may be taken on another side than float64 takes it only where float64's input lies within
2e-4, relative, of zero; everything but the moved tensors' gradients bitwise a bf16x3wa step's; repeats on dirty scratch; the switches back.
"""

import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import transformer_bf16x3w_forms as W
import transformer_bf16x3wac_forms as WC
import transformer_ragged_oracle as R
import transformer_train_bf16x3_emulation as E
import transformer_train_bf16x3wac_emulation as EC
import transformer_train_oracle as O
from test_gpu_transformer_packed import native_packed_step, pstep
from test_gpu_transformer_ragged import native_step, padded
from test_gpu_transformer_train import assert_within, batch_of, dev, step, steps_config
from test_transformer_train_bf16x3wac_host import N_SPLIT_CASES, split_cases
from articulatory_amd import _native
from articulatory_amd.bin.train import InversionTrainer
from articulatory_amd.models import Transformer
from articulatory_amd.models.transformer import _grad_layout
from articulatory_amd.utils.synth import uniform

pytestmark = pytest.mark.gpu

REFERENCE_ON_THE_DEVICE = ("rows4112",)  # as tests/test_gpu_transformer_train_edges.py, which holds that float64 run to the host's
G_SPLIT, A_SPLIT = "xfmr_split_rows_t_kernel", "xfmr_split_taps_t_kernel"
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
        shapes = WC.case_shapes(name)
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


def row_shape(row):
    """(cout, cin, K) of a weight-gradient or reduction row under HIFICAR_PROFILE_DETAIL=1 ('kernel CxIkK[pP] ...')."""
    cout, rest = row.split(" ")[1].split("x")
    cin, rest = rest.split("k")
    return int(cout), int(cin), int(rest.split("p")[0])


def check_rows(name, form, rows_c, rows_a):
    """The profile of a bf16x3wac step (rows_c) by name, both ways, against the restated rule and against the bf16x3wa step's (rows_a)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    moved, onetap, rest = WC.case_launches(name, form, num_cus=cus)
    assert moved and onetap and rest
    moved_shapes = collections.Counter((l.layer.cout, l.layer.cin, 3) for l in moved)
    # exactly the selected convs in wgrad_bf16x3_kernel<4,32> under their own k3 shape, each with the one-tap twin's split
    got = {}
    for r, n in rows_c.items():
        if r.startswith("wgrad_bf16x3_kernel") and row_shape(r)[2] == 3:
            _, _, s, key = W.parse_row(r)
            assert key not in got, r
            got[key] = (n, s)
    assert got == WC.expected_rows(moved), (name, form, got, WC.expected_rows(moved))
    # ... none of them in wgrad_taps_kernel any more; the fp32 rows are the rest's, all of it; the one-tap rows are bf16x3wa's own
    other = collections.Counter()
    for r, n in rows_c.items():
        if r.startswith("wgrad_") and not r.startswith("wgrad_bf16x3_kernel"):
            other[row_shape(r)] += n
    assert other == collections.Counter((L.cout, L.cin, L.K) for L in rest), (name, form, other)
    assert not any(r.startswith("wgrad_taps_kernel") and row_shape(r) in moved_shapes for r in rows_c)
    k1 = lambda rows: {r: n for r, n in rows.items() if r.startswith("wgrad_bf16x3_kernel") and row_shape(r)[2] == 1}  # noqa: E731
    assert k1(rows_c) == k1(rows_a) and sum(k1(rows_c).values()) == len(onetap)
    # the bf16x3wa step: the same convs in wgrad_taps_kernel, no k3 GEMM row, no tap-column split
    taps_a = collections.Counter()
    for r, n in rows_a.items():
        assert not (r.startswith("wgrad_bf16x3_kernel") and row_shape(r)[2] == 3), r
        if r.startswith("wgrad_taps_kernel") and row_shape(r) in moved_shapes:
            taps_a[row_shape(r)] += n
    assert taps_a == moved_shapes, (name, form, taps_a)
    # one G split and one tap-column split per moved layer, beside bf16x3w's two per one-tap layer
    assert rows_c.get(A_SPLIT, 0) == len(moved) and A_SPLIT not in rows_a
    assert rows_a.get(G_SPLIT, 0) == 2 * len(onetap) and rows_c.get(G_SPLIT, 0) == 2 * len(onetap) + len(moved)
    # every other row — the moved layers' launches, their reductions and the two split passes aside — equals the bf16x3wa step's
    def others(rows):
        return {r: n for r, n in rows.items() if r not in (G_SPLIT, A_SPLIT) and not (r.startswith(("wgrad_", "wreduce_")) and row_shape(r) in moved_shapes)}
    assert others(rows_c) == others(rows_a), (name, form, set(others(rows_c).items()) ^ set(others(rows_a).items()))
    reduced = lambda rows: sum(n for r, n in rows.items() if r.startswith("wreduce_") and row_shape(r) in moved_shapes)  # noqa: E731
    assert reduced(rows_c) == reduced(rows_a) == len(moved)
    assert any(r.startswith("xfmr_attn16") for r in rows_c) and any(r.startswith("conv_bf16x3") for r in rows_c)


def assert_same_but_the_moved_gradients(c, a, params, what):
    """Two steps in the restatement's layout: everything bitwise equal but the gradients bf16x3wac moved to bf16 MFMAs, which differ."""
    assert torch.equal(c["out"], a["out"]) and torch.equal(c["loss"], a["loss"]) and torch.equal(c["dx"], a["dx"]) and torch.equal(c["stats"], a["stats"]), what
    assert all(torch.equal(c["running"][k], v) for k, v in a["running"].items()), what
    moved = set(WC.moved_tensors(params))
    assert moved <= set(c["grads"]) == set(a["grads"])
    for k, g in a["grads"].items():
        assert torch.isfinite(c["grads"][k]).all() and torch.equal(c["grads"][k], g) == (k not in moved), (what, k)


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
    """One bf16x3wac step of a dense case, the float64 reference on its ReLU sides, a second model's step with its profile, and the bf16x3wa
    step of the same model and seed with its profile: computed once per module and left unchanged."""
    if name not in _RUNS:
        params, sd, x, t, shapes = case(name)
        mc = model(params, sd, "bf16x3wac")
        gates = {}
        got = step(mc, x, t, gates=gates)
        ref = O.restatement(name, torch.float64, device="cuda:0" if name in REFERENCE_ON_THE_DEVICE else "cpu", gates=gates, shapes=shapes)
        mc2 = model(params, sd, "bf16x3wac")
        again, rows_c = profiled(mc2, lambda: step(mc2, x, t))
        ma = model(params, sd, "bf16x3wa")
        x3wa, rows_a = profiled(ma, lambda: step(ma, x, t))
        _RUNS[name] = dict(got=got, ref=ref, again=again, rows_c=rows_c, x3wa=x3wa, rows_a=rows_a)
    return _RUNS[name]


# ------------------------------------------------------------------------------------------------ the dense cases
@pytest.mark.parametrize("name", WC.DENSE_CASES)
def test_profile_rows_by_name_both_ways(name):
    r = run(name)
    print("  " + "\n  ".join(sorted(k for k in r["rows_c"] if k.startswith(("wgrad_", "wreduce_", "xfmr_split_rows_t", "xfmr_split_taps_t")))))
    check_rows(name, "dense", r["rows_c"], r["rows_a"])


@pytest.mark.parametrize("name", WC.DENSE_CASES)
def test_step_against_the_restatement(name):
    r = run(name)
    got, ref = r["got"], r["ref"]
    print(f"  {name}: {ref['gate_flips']} ReLU(s) on the other side than float64's own, the farthest {ref['gate_gap']:.3g} of max |x| from zero")
    assert ref["gate_gap"] < E.X3_OUT_BAR
    assert set(got["grads"]) == set(ref["grads"])
    errs = EC.errors_x3wac(got, ref)
    moved = ["grad." + k for k in WC.moved_tensors(case(name)[0])]
    print("  the moved tensors' worst: %s" % ", ".join(f"{k} {errs[k][0]:.3g}" for k in sorted(moved, key=lambda k: -errs[k][0])[:3]))
    assert_within(errs, name)
    assert torch.isfinite(got["out"]).all() and torch.isfinite(got["dx"]).all()
    assert "libhificar.so" in open("/proc/self/maps").read()


@pytest.mark.parametrize("name", WC.DENSE_CASES)
def test_everything_else_is_bitwise_the_bf16x3wa_step_and_repeats_are_bit_identical(name):
    r = run(name)
    params = case(name)[0]
    assert_same_but_the_moved_gradients(r["got"], r["x3wa"], params, name)
    assert_equal_steps(r["got"], r["again"], name + " on a second model")  # (with and without the debug taps)
    # the moved gradients differ from the fp32 kernels' by rounding, not by more: both lie within the bar of float64, so within two of each other
    for k in WC.moved_tensors(params):
        d = float((r["got"]["grads"][k] - r["x3wa"]["grads"][k]).abs().max()) / O.grad_scale(r["ref"]["grads"], k)
        assert 0 < d < 2 * EC.BARS_X3WAC["grad"], (name, k, d)


@pytest.mark.parametrize("name", WC.DENSE_CASES)
def test_dirty_scratch_equal_lengths_and_the_switches_back(name):
    params, sd, x, t, _ = case(name)
    B, _, T = x.shape
    p, seed = params["dropout"], O.SEEDS[name]
    m = model(params, sd, "bf16x3wac")
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
    # the same handle switched to bf16x3wa, then to f32: the next steps are those of fresh models in those arithmetics, bitwise
    for arithmetic in ("bf16x3wa", "f32"):
        m.set_train_precision(arithmetic)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)  # (the running statistics moved)
        m.set_dropout_seed(O.DROPOUT_SEED)
        fresh = run(name)["x3wa"] if arithmetic == "bf16x3wa" else step(model(params, sd, "f32"), x, t)
        assert_equal_steps(step(m, x, t), fresh, f"{name} after set_train_precision({arithmetic})")


def test_a_switch_from_bf16x3wa_rebuilds_nothing():
    name = "t65"
    params, sd, x, t, _ = case(name)
    ma = model(params, sd, "bf16x3wa")
    step(ma, x, t)
    ma.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    ma.set_dropout_seed(O.DROPOUT_SEED)
    ma._native_handle(train=True)  # (the hand-over of the reloaded parameters, in bf16x3wa: the tables are split here)
    _, rows = profiled(ma, lambda: ma.set_train_precision("bf16x3wac"))
    assert rows == {}, rows  # no weight pack, no table
    assert_equal_steps(step(ma, x, t), run(name)["got"], "bf16x3wa -> bf16x3wac")
    # from bf16x3w the tables are split, as towards bf16x3wa
    mw = model(params, sd, "bf16x3w")
    step(mw, x, t)
    mw.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    mw.set_dropout_seed(O.DROPOUT_SEED)
    mw._native_handle(train=True)
    _, rows = profiled(mw, lambda: mw.set_train_precision("bf16x3wac"))
    assert rows == {"xfmr_split_tab_kernel": params["elayers"]}, rows
    assert_equal_steps(step(mw, x, t), run(name)["got"], "bf16x3w -> bf16x3wac")


def test_a_backward_after_a_switch_is_refused_and_the_tape_survives():
    name = "t65"
    params, sd, x, t, _ = case(name)
    straight = run(name)["got"]
    m = model(params, sd, "bf16x3wac")
    xt = dev(x).requires_grad_(True)
    loss = F.l1_loss(m(xt), dev(t))
    for other in ("bf16x3wa", "bf16x3w", "bf16x3", "f32"):
        m.set_train_precision(other)
        with pytest.raises(RuntimeError, match=f"training arithmetic is {other}, its last training forward ran in bf16x3wac"):
            loss.backward(retain_graph=True)
        assert xt.grad is None and all(q.grad is None for q in m.parameters())
    m.set_train_precision("bf16x3wac")
    loss.backward()
    assert torch.equal(xt.grad, straight["dx"]) and all(torch.equal(q.grad, straight["grads"][k]) for k, q in m.named_parameters())
    # ... and the other way round: a bf16x3wa tape does not go back through bf16x3wac
    ma = model(params, sd, "bf16x3wa")
    loss = F.l1_loss(ma(dev(x)), dev(t))
    ma.set_train_precision("bf16x3wac")
    with pytest.raises(RuntimeError, match="training arithmetic is bf16x3wac, its last training forward ran in bf16x3wa "):
        loss.backward()


@pytest.mark.parametrize("name", ["t65", "nores", "d48"])
def test_workspace_and_tape_are_those_of_bf16x3wa(name):
    params, sd, _, _, _ = case(name)
    m = model(params, sd, "bf16x3wa")
    m._native_handle(train=True)
    lib, h = m._lib, m._handle
    host = torch.tensor([70, 33, 1], dtype=torch.int32)
    mp = lib.hificar_xfmr_packed_rows(3, 70, host.data_ptr())
    sizes = lambda: (lib.hificar_xfmr_train_workspace_bytes(h, 2, 65), lib.hificar_xfmr_train_workspace_bytes_packed(h, 3, mp),  # noqa: E731
                     lib.hificar_xfmr_train_workspace_bytes(h, 16, 257), lib.hificar_xfmr_tape_bytes(h, 2, 65), lib.hificar_xfmr_tape_bytes_packed(h, 3, mp))
    x3wa = sizes()
    m.set_train_precision("bf16x3wac")
    assert sizes() == x3wa and all(x3wa)  # A3 goes into the second of bf16x3w's split buffers; the GEMM form's partials fit the one-tap layers'


# ------------------------------------------------------------------------------------------------ the ragged batches, padded and packed
def ragged_model(name, arithmetic):
    params, sd, x, t, lengths = R.ragged_case(name)
    return model(params, sd, arithmetic), params, x, t, lengths


@pytest.mark.parametrize("form", ["ragged", "packed"])
@pytest.mark.parametrize("name", WC.RAGGED_CASES)
def test_ragged_and_packed_steps(name, form):
    m, params, x, t, lengths = ragged_model(name, "bf16x3wac")
    gates = {}
    got = pstep(m, x, t, lengths, form=form, gates=gates)
    ref = R.ragged_restatement(name, torch.float64, gates=gates)
    print(f"  {name} {form}: {ref['gate_flips']} ReLU(s) on the other side than float64's own, the farthest {ref['gate_gap']:.3g} of max |x| from zero")
    assert ref["gate_gap"] < E.X3_OUT_BAR
    assert_within(EC.errors_x3wac(got, ref), f"{name} {form}")
    assert float(padded(got["out"], lengths).abs().max()) == 0.0 and float(padded(got["dx"], lengths).abs().max()) == 0.0
    mc, ma = ragged_model(name, "bf16x3wac")[0], ragged_model(name, "bf16x3wa")[0]
    again, rows_c = profiled(mc, lambda: pstep(mc, x, t, lengths, form=form))
    x3wa, rows_a = profiled(ma, lambda: pstep(ma, x, t, lengths, form=form))
    check_rows(name, form, rows_c, rows_a)
    assert_equal_steps(got, again, f"{name} {form} on a second model")
    assert_same_but_the_moved_gradients(got, x3wa, params, f"{name} {form}")
    for k in WC.moved_tensors(params):
        d = float((got["grads"][k] - x3wa["grads"][k]).abs().max()) / O.grad_scale(ref["grads"], k)
        assert 0 < d < 2 * EC.BARS_X3WAC["grad"], (name, form, k, d)


@pytest.mark.parametrize("name", WC.RAGGED_CASES)
def test_nan_on_padded_frames_and_dirty_scratch_change_nothing(name):
    m, params, x, _, lengths = ragged_model(name, "bf16x3wac")
    m._native_handle(train=True)
    B, _, T = x.shape
    p, seed = params["dropout"], R.RAGGED_SEEDS[name]
    x = dev(x)
    dout = dev(uniform(seed, "dout", (B, params["out_channels"], T), -1.0, 1.0))
    dense = native_step(m, x, dout, p, 0x00)
    # zeros on padded frames; NaN there in x and dout, on 0xFF-filled buffers, changes nothing: both split passes write such rows, and the
    # taps that reach into them, as zero bits without reading them
    pad = (~R.valid_mask(lengths, T)).to("cuda:0")[:, None, :]
    xz, dz = x.masked_fill(pad, 0.0).contiguous(), dout.masked_fill(pad, 0.0).contiguous()
    xn, dn = x.masked_fill(pad, float("nan")).contiguous(), dout.masked_fill(pad, float("nan")).contiguous()
    for what, fn in (("ragged", lambda *a: native_step(m, *a, lengths=lengths)), ("packed", lambda *a: native_packed_step(m, *a, lengths))):
        clean, dirty = fn(xz, dz, p, 0x00), fn(xn, dn, p, 0xFF)
        same(clean, dirty, m, what)
        assert float(padded(dirty[0], lengths).abs().max()) == 0.0 and float(padded(dirty[3], lengths).abs().max()) == 0.0, what
        assert not torch.equal(clean[0], dense[0])


# ------------------------------------------------------------------------------------------------ five steps through the trainer
def test_five_steps_through_the_trainer_then_back_to_bf16x3wa():
    params, sd, _, _ = O.case(O.STEPS_CASE)
    tr = InversionTrainer(dict(steps_config(params), train_precision="bf16x3wac"), torch.device("cuda:0"))
    tr.G.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    tr.G.set_dropout_seed(O.DROPOUT_SEED)
    assert tr.G.train_precision == "bf16x3wac" and tr.optimizer["generator"].defaults.get("fused") is True
    losses = [float(tr.train_step(batch_of(s))["train/generator_loss"]) for s in range(O.STEPS["n"])]
    ref_losses, ref_final = O.five_steps(torch.float64)
    e_loss, worst = O.five_step_errors(losses, dict(tr.G.state_dict()), ref_losses, ref_final)
    print("losses", losses, "deviation", e_loss, "worst final tensor", max(worst, key=worst.get), max(worst.values()))
    assert e_loss < EC.BARS_X3WAC["steps_loss"]
    assert max(worst.values()) < EC.BARS_X3WAC["steps_params"]
    # back to bf16x3wa on the same handle: the next step is a fresh bf16x3wa model's on the same state_dict, bitwise
    tr.G.set_train_precision("bf16x3wa")
    fresh = Transformer(train_precision="bf16x3wa", **params)
    fresh.load_state_dict(tr.G.state_dict(), strict=True)
    fresh = fresh.to("cuda:0").train()
    fresh.set_dropout_seed(O.DROPOUT_SEED, offset=tr.G._calls)
    _, _, x, t = O.case(O.STEPS_CASE, 7)
    assert_equal_steps(step(tr.G, x, t), step(fresh, x, t), "after five bf16x3wac steps")


# ------------------------------------------------------------------------------------------------ the split pass on the device
def test_device_tap_column_bytes_are_the_numpy_restatement():
    """xfmr_split_taps_t_kernel over a buffer of 0xFF bytes against the layout's numpy restatement, byte for byte: the host test's cases."""
    seen = 0
    for what, got, want in split_cases(1):
        assert got.shape == want.shape and np.array_equal(got, want), what
        seen += 1
    assert seen == N_SPLIT_CASES
