"""The Transformer's opt-in bf16x3wa training arithmetic on a MI355X (``train_precision="bf16x3wa"``: the bf16x3w step with the training
attention's query-tiled kernels — xfmr_attn16_train_kernel and xfmr_attn16_bwd_q_kernel — on bf16 MFMAs; the key-tiled kernels stay fp32).
``pytest -m gpu``.

Per case (tests/transformer_train_bf16x3wa_emulation.py: ALL_DENSE — head size 16 at the tile and band edges, and one case per template
instantiation, 48 / 80 / 112 with a zero-padded contraction — and RAGGED_CASES, each padded and packed): the profile rows by name, both
ways, against a bf16x3w step's; every quantity against the float64 restatement on the device's own ReLU sides, within BARS_X3WA — set on the
CPU before the first GPU run, tests/test_transformer_train_bf16x3wa_host.py holds the emulation to a quarter of them; a ReLU may be taken on
another side than float64 takes it only where float64's input lies within 2e-4, relative, of zero; what lies upstream of the first attention
bitwise a bf16x3w step's.  On a subset: repeats on dirty scratch around a step of another shape, NaN on padded frames, the switches.
"""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import transformer_ragged_oracle as R
import transformer_train_bf16x3_emulation as E
import transformer_train_bf16x3wa_emulation as EA
import transformer_train_oracle as O
from test_gpu_transformer_packed import native_packed_step, pstep
from test_gpu_transformer_ragged import native_step, padded
from test_gpu_transformer_train import assert_within, batch_of, dev, step, steps_config
from articulatory_amd import _native
from articulatory_amd.bin.train import InversionTrainer
from articulatory_amd.models import Transformer
from articulatory_amd.models.transformer import _grad_layout
from articulatory_amd.utils.synth import uniform

pytestmark = pytest.mark.gpu

OLD_ROWS = ("xfmr_attn_kernel<train>", "xfmr_attn_bwd_kernels")                                     # the three older arithmetics' attention
NEW_ROWS = ("xfmr_attn16_kernel<train>", "xfmr_attn16_bwd_q_kernel", "xfmr_attn_bwd_k_kernels")    # bf16x3wa's: forward, backward-q, the fp32 rest
TAB_ROW = "xfmr_split_tab_kernel"                                                                   # the tables' split, one per layer and hand-over
_CASES, _RUNS, _RAGGED = {}, {}, {}


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


def check_rows(what, rows_a, rows_w, elayers):
    """The profile of a bf16x3wa step (rows_a) by name, both ways, against the bf16x3w step's on the same case (rows_w): a model's first step,
    so one parameter hand-over lies inside it."""
    for r in NEW_ROWS:
        assert rows_a.get(r, 0) == elayers and r not in rows_w, (what, r)       # one per layer, and only here
    for r in OLD_ROWS:
        assert r not in rows_a and rows_w.get(r, 0) == elayers, (what, r)       # none of the fp32 query-tiled launches
    assert rows_a.get(TAB_ROW, 0) == elayers and TAB_ROW not in rows_w, what    # the one new row beside them: no split pass over q | k | v
    drop = OLD_ROWS + NEW_ROWS + (TAB_ROW,)
    rest_a, rest_w = ({r: n for r, n in rows.items() if r not in drop} for rows in (rows_a, rows_w))
    assert rest_a == rest_w, (what, set(rest_a.items()) ^ set(rest_w.items()))
    assert any(r.startswith("wgrad_bf16x3_kernel") for r in rest_a) and any(r.startswith("conv_bf16x3") for r in rest_a)


def assert_upstream_equal_and_the_rest_moved(a, w, what):
    """A bf16x3wa step against a bf16x3w step on the same inputs: the conv_blocks batch statistics and running buffers lie upstream of the
    first attention and are equal to the bit; out is not; every gradient is finite."""
    assert torch.equal(a["stats"], w["stats"]) and all(torch.equal(a["running"][k], v) for k, v in w["running"].items()), what
    assert not torch.equal(a["out"], w["out"]), what
    assert torch.isfinite(a["out"]).all() and torch.isfinite(a["dx"]).all() and set(a["grads"]) == set(w["grads"]), what
    assert all(torch.isfinite(g).all() for g in a["grads"].values()), what


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
    """One bf16x3wa step of a dense case, the float64 reference on its ReLU sides, a second model's step with its profile, and the bf16x3w
    step of the same model and seed with its profile: computed once per module and left unchanged."""
    if name not in _RUNS:
        params, sd, x, t, shapes = case(name)
        ma = model(params, sd, "bf16x3wa")
        gates = {}
        got = step(ma, x, t, gates=gates)
        ref = O.restatement(name, torch.float64, gates=gates, shapes=shapes)
        ma2 = model(params, sd, "bf16x3wa")
        again, rows_a = profiled(ma2, lambda: step(ma2, x, t))
        mw = model(params, sd, "bf16x3w")
        x3w, rows_w = profiled(mw, lambda: step(mw, x, t))
        _RUNS[name] = dict(got=got, ref=ref, again=again, rows_a=rows_a, x3w=x3w, rows_w=rows_w)
    return _RUNS[name]


# ------------------------------------------------------------------------------------------------ the dense cases
@pytest.mark.parametrize("name", EA.ALL_DENSE)
def test_profile_rows_by_name_both_ways(name):
    r = run(name)
    print("  " + "\n  ".join(sorted(k for k in r["rows_a"] if "attn" in k or k == TAB_ROW)))
    check_rows(name, r["rows_a"], r["rows_w"], case(name)[0]["elayers"])


@pytest.mark.parametrize("name", EA.ALL_DENSE)
def test_step_against_the_restatement(name):
    r = run(name)
    got, ref = r["got"], r["ref"]
    print(f"  {name}: {ref['gate_flips']} ReLU(s) on the other side than float64's own, the farthest {ref['gate_gap']:.3g} of max |x| from zero")
    assert ref["gate_gap"] < E.X3_OUT_BAR
    assert set(got["grads"]) == set(ref["grads"])
    assert_within(EA.errors_x3wa(got, ref), name)
    assert "libhificar.so" in open("/proc/self/maps").read()


@pytest.mark.parametrize("name", EA.ALL_DENSE)
def test_against_the_bf16x3w_step_and_a_second_model(name):
    r = run(name)
    assert_upstream_equal_and_the_rest_moved(r["got"], r["x3w"], name)
    assert_equal_steps(r["got"], r["again"], name + " on a second model")  # (with and without the debug taps)
    # out moved by rounding, not by more: both lie within the output bar of float64
    d = float((r["got"]["out"] - r["x3w"]["out"]).abs().max() / r["ref"]["out"].abs().max())
    assert 0 < d < 2 * EA.BARS_X3WA["out"], (name, d)


@pytest.mark.parametrize("name", ["t65", "d48", "d128"])
def test_dirty_scratch_around_a_step_of_another_shape(name):
    params, sd, x, _, _ = case(name)
    B, _, T = x.shape
    p, seed = params["dropout"], O.SEEDS[name]
    m = model(params, sd, "bf16x3wa")
    m._native_handle(train=True)
    xd = dev(x)
    dout = dev(uniform(seed, "dout", (B, params["out_channels"], T), -1.0, 1.0))
    first = native_step(m, xd, dout, p, 0xFF)
    T2 = T - 7  # (another tile count or another ragged last tile; other buffers, the same handle)
    native_step(m, xd[:, :, :T2].contiguous(), dout[:, :, :T2].contiguous(), p, 0xFF)
    same(first, native_step(m, xd, dout, p, 0x00), m, "after a step of another shape, zero-filled buffers")
    same(first, native_step(m, xd, dout, p, 0xFF, lengths=[T] * B), m, "every length = T")
    assert float(first[3].abs().max()) > 0


def test_the_switches_back_give_fresh_models_steps():
    name = "t65"
    params, sd, x, t, _ = case(name)
    m = model(params, sd, "bf16x3wa")
    assert_equal_steps(step(m, x, t), run(name)["got"], name)
    for arithmetic in ("bf16x3w", "f32", "bf16x3wa"):
        m.set_train_precision(arithmetic)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)  # (the running statistics moved)
        m.set_dropout_seed(O.DROPOUT_SEED)
        fresh = {"bf16x3w": lambda: run(name)["x3w"], "bf16x3wa": lambda: run(name)["got"], "f32": lambda: step(model(params, sd, "f32"), x, t)}[arithmetic]()
        assert_equal_steps(step(m, x, t), fresh, f"{name} after set_train_precision({arithmetic})")
    # bf16x3w -> bf16x3wa on a handle that has its parameters: the tables are split behind the switch, no hand-over in between
    mw = model(params, sd, "bf16x3w")
    step(mw, x, t)
    mw.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    mw.set_dropout_seed(O.DROPOUT_SEED)
    mw._native_handle(train=True)  # (the hand-over of the reloaded parameters, in bf16x3w)
    _, rows = profiled(mw, lambda: mw.set_train_precision("bf16x3wa"))
    assert rows == {TAB_ROW: params["elayers"]}, rows  # no weight pack is rebuilt
    assert_equal_steps(step(mw, x, t), run(name)["got"], "bf16x3w -> bf16x3wa")


def test_a_backward_after_a_switch_is_refused_and_the_tape_survives():
    name = "t65"
    params, sd, x, t, _ = case(name)
    straight = run(name)["got"]
    m = model(params, sd, "bf16x3wa")
    xt = dev(x).requires_grad_(True)
    loss = F.l1_loss(m(xt), dev(t))
    for other in ("bf16x3w", "bf16x3", "f32"):
        m.set_train_precision(other)
        with pytest.raises(RuntimeError, match=f"training arithmetic is {other}, its last training forward ran in bf16x3wa"):
            loss.backward(retain_graph=True)
        assert xt.grad is None and all(q.grad is None for q in m.parameters())
    m.set_train_precision("bf16x3wa")
    loss.backward()
    assert torch.equal(xt.grad, straight["dx"]) and all(torch.equal(q.grad, straight["grads"][k]) for k, q in m.named_parameters())
    # ... and the other way round: a bf16x3w tape does not go back through bf16x3wa
    mw = model(params, sd, "bf16x3w")
    loss = F.l1_loss(mw(dev(x)), dev(t))
    mw.set_train_precision("bf16x3wa")
    with pytest.raises(RuntimeError, match="training arithmetic is bf16x3wa, its last training forward ran in bf16x3w "):
        loss.backward()


def test_workspace_and_tape_are_those_of_bf16x3w():
    params, sd, _, _, _ = case("t65")
    m = model(params, sd, "bf16x3w")
    m._native_handle(train=True)
    lib, h = m._lib, m._handle
    host = torch.tensor([70, 33, 1], dtype=torch.int32)
    mp = lib.hificar_xfmr_packed_rows(3, 70, host.data_ptr())
    sizes = lambda: (lib.hificar_xfmr_train_workspace_bytes(h, 2, 65), lib.hificar_xfmr_train_workspace_bytes_packed(h, 3, mp),  # noqa: E731
                     lib.hificar_xfmr_tape_bytes(h, 2, 65), lib.hificar_xfmr_tape_bytes_packed(h, 3, mp))
    x3w = sizes()
    m.set_train_precision("bf16x3wa")
    assert sizes() == x3w and all(x3w)  # the keys are split on their way into LDS, the tables into handle state: no scratch of this arithmetic's own


# ------------------------------------------------------------------------------------------------ the ragged batches, padded and packed
def ragged_model(name, arithmetic):
    params, sd, x, t, lengths = R.ragged_case(name)
    return model(params, sd, arithmetic), params, x, t, lengths


@pytest.mark.parametrize("form", ["ragged", "packed"])
@pytest.mark.parametrize("name", EA.RAGGED_CASES)
def test_ragged_and_packed_steps(name, form):
    m, params, x, t, lengths = ragged_model(name, "bf16x3wa")
    gates = {}
    got = pstep(m, x, t, lengths, form=form, gates=gates)
    ref = R.ragged_restatement(name, torch.float64, gates=gates)
    print(f"  {name} {form}: {ref['gate_flips']} ReLU(s) on the other side than float64's own, the farthest {ref['gate_gap']:.3g} of max |x| from zero")
    assert ref["gate_gap"] < E.X3_OUT_BAR
    assert_within(EA.errors_x3wa(got, ref), f"{name} {form}")
    assert float(padded(got["out"], lengths).abs().max()) == 0.0 and float(padded(got["dx"], lengths).abs().max()) == 0.0
    ma, mw = ragged_model(name, "bf16x3wa")[0], ragged_model(name, "bf16x3w")[0]
    again, rows_a = profiled(ma, lambda: pstep(ma, x, t, lengths, form=form))
    x3w, rows_w = profiled(mw, lambda: pstep(mw, x, t, lengths, form=form))
    check_rows(f"{name} {form}", rows_a, rows_w, params["elayers"])
    assert_equal_steps(got, again, f"{name} {form} on a second model")
    assert_upstream_equal_and_the_rest_moved(got, x3w, f"{name} {form}")


def test_nan_on_padded_frames_changes_nothing_padded_and_packed():
    name = "mixed"
    m, params, x, _, lengths = ragged_model(name, "bf16x3wa")
    m._native_handle(train=True)
    B, _, T = x.shape
    p, seed = params["dropout"], R.RAGGED_SEEDS[name]
    x = dev(x)
    dout = dev(uniform(seed, "dout", (B, params["out_channels"], T), -1.0, 1.0))
    dense = native_step(m, x, dout, p, 0x00)
    # zeros on padded frames; NaN there in x and dout, on 0xFF-filled buffers, gives the same bits: rows past a length and gap rows are never
    # read as data by the new kernels (the staging writes zeros for them), and their own rows come out as zeros
    pad = (~R.valid_mask(lengths, T)).to("cuda:0")[:, None, :]
    xz, dz = x.masked_fill(pad, 0.0).contiguous(), dout.masked_fill(pad, 0.0).contiguous()
    xn, dn = x.masked_fill(pad, float("nan")).contiguous(), dout.masked_fill(pad, float("nan")).contiguous()
    for what, fn in (("ragged", lambda *a: native_step(m, *a, lengths=lengths)), ("packed", lambda *a: native_packed_step(m, *a, lengths))):
        clean, dirty = fn(xz, dz, p, 0x00), fn(xn, dn, p, 0xFF)
        same(clean, dirty, m, what)
        assert float(padded(dirty[0], lengths).abs().max()) == 0.0 and float(padded(dirty[3], lengths).abs().max()) == 0.0, what
        assert not torch.equal(clean[0], dense[0])


# ------------------------------------------------------------------------------------------------ five steps through the trainer
def test_five_steps_through_the_trainer():
    params, sd, _, _ = O.case(O.STEPS_CASE)
    tr = InversionTrainer(dict(steps_config(params), train_precision="bf16x3wa"), torch.device("cuda:0"))
    tr.G.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    tr.G.set_dropout_seed(O.DROPOUT_SEED)
    assert tr.G.train_precision == "bf16x3wa" and tr.optimizer["generator"].defaults.get("fused") is True
    losses = [float(tr.train_step(batch_of(s))["train/generator_loss"]) for s in range(O.STEPS["n"])]
    ref_losses, ref_final = O.five_steps(torch.float64)
    e_loss, worst = O.five_step_errors(losses, dict(tr.G.state_dict()), ref_losses, ref_final)
    print("losses", losses, "deviation", e_loss, "worst final tensor", max(worst, key=worst.get), max(worst.values()))
    assert e_loss < EA.BARS_X3WA["steps_loss"]
    assert max(worst.values()) < EA.BARS_X3WA["steps_params"]
