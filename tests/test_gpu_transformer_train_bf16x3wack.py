"""The Transformer's opt-in bf16x3wack training arithmetic on a MI355X (``train_precision="bf16x3wack"``: the bf16x3wac step, and the attention's
key-tiled backward — xfmr_attn16_bwd_k_kernel for dK and dV, xfmr_demb16_partial_kernel for the first stage of the tables' gradient — on bf16
MFMAs).  ``pytest -m gpu``.

Per case (transformer_train_bf16x3wack_emulation: DENSE_CASES — head size 16 at the tile and band edges —, HEAD_CASES — one per template
instantiation — and the RAGGED_CASES padded and packed): the profile rows by name, both ways, against a bf16x3wac step's; every quantity against
the float64 restatement on the device's own ReLU sides, within BARS_X3WACK — set on the CPU before the first GPU run,
tests/test_transformer_train_bf16x3wack_host.py holds the emulation to a quarter of them; out, the tape a training forward leaves (which holds
L), and what the backward computes before the key-tiled kernels run, bitwise a bf16x3wac step's.  The last layer's dQ lives in the workspace
only, so it is read through the one gradient it alone feeds: the last layer's w_q gradient is dQ^T X in a GEMM whose other columns (dK, dV) do
not enter those rows.  On a subset: repeats, dirty scratch around a step of another shape, NaN on padded frames, five steps through the trainer
under the config key, the switches between arithmetics on one model.
"""

import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import transformer_ragged_oracle as R
import transformer_train_bf16x3_emulation as E
import transformer_train_bf16x3wack_emulation as EK
import transformer_train_oracle as O
from test_gpu_bigru_train_edges import owned, owned_floats
from test_gpu_transformer_packed import native_packed_step, pstep
from test_gpu_transformer_ragged import native_step, padded
from test_gpu_transformer_train import assert_within, batch_of, dev, step, steps_config
from articulatory_amd import _native
from articulatory_amd.bin.train import InversionTrainer
from articulatory_amd.models import Transformer
from articulatory_amd.models.transformer import _grad_layout
from articulatory_amd.utils.synth import uniform

pytestmark = pytest.mark.gpu

OLD_ROW = "xfmr_attn_bwd_k_kernels"                                    # bf16x3wa's and bf16x3wac's key-tiled pair, exact fp32
NEW_ROWS = ("xfmr_attn16_bwd_k_kernel", "xfmr_demb16_partial_kernel")  # bf16x3wack's
MOVED = ("self_attn.w_k", "self_attn.w_v", "self_attn.relative_positional.embeddings")  # of the last layer: what the pair feeds and nothing above it does
_CASES, _RUNS = {}, {}


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


def check_rows(what, rows_k, rows_c, elayers):
    """The profile of a bf16x3wack step (rows_k) by name, both ways, against the bf16x3wac step's on the same case (rows_c)."""
    for r in NEW_ROWS:
        assert rows_k.get(r, 0) == elayers and r not in rows_c, (what, r)  # one per layer, and only here
    assert OLD_ROW not in rows_k and rows_c.get(OLD_ROW, 0) == elayers, what   # none of the fp32 key-tiled launches
    drop = NEW_ROWS + (OLD_ROW,)
    rest_k, rest_c = ({r: n for r, n in rows.items() if r not in drop} for rows in (rows_k, rows_c))
    assert rest_k == rest_c, (what, set(rest_k.items()) ^ set(rest_c.items()))
    assert rest_k.get("xfmr_attn16_bwd_q_kernel", 0) == elayers and rest_k.get("bigru_colreduce_kernel", 0) == rest_c.get("bigru_colreduce_kernel", 0)


def assert_equal_steps(a, b, what):
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["dx"], b["dx"]) and torch.equal(a["stats"], b["stats"]), what
    assert set(a["grads"]) == set(b["grads"]) and all(torch.equal(a["grads"][k], g) for k, g in b["grads"].items()), what


def assert_bitwise_up_to_the_key_tiled_kernels(k, c, ref, params, what):
    """A bf16x3wack step (k) against a bf16x3wac step (c) on the same inputs: the forward's results and everything the backward computes before
    the last layer's key-tiled kernels run are equal to the bit — the last layer's w_q gradient stands for its dQ —; what those kernels feed
    differs from the fp32 pair's by rounding, not by more: both lie within the bar of float64, so within two of each other."""
    assert torch.equal(k["out"], c["out"]) and torch.equal(k["loss"], c["loss"]) and torch.equal(k["stats"], c["stats"]), what
    assert all(torch.equal(k["running"][n], v) for n, v in c["running"].items()), what
    assert set(k["grads"]) == set(c["grads"]) and all(torch.isfinite(g).all() for g in k["grads"].values()) and torch.isfinite(k["dx"]).all(), what
    last = f"transformer.layers.{params['elayers'] - 1}."
    moved = [last + t for t in MOVED]
    above = [n for n in k["grads"] if (n.startswith(last) or n.startswith("w_out.")) and n not in moved]
    assert last + "self_attn.w_q" in above and last + "self_attn.w_o" in above and len(above) >= 10, above
    for n in above:
        assert torch.equal(k["grads"][n], c["grads"][n]), (what, n)
    worst = 0.0
    for n in moved:
        d = float((k["grads"][n] - c["grads"][n]).abs().max()) / O.grad_scale(ref["grads"], n)
        assert d < 2 * EK.BARS_X3WACK["grad"], (what, n, d)
        worst = max(worst, d)
    assert worst > 0 and not torch.equal(k["dx"], c["dx"]), what  # the new kernels ran, and their results reach the input


def tape_after_forward(m, x, p, lengths=None, form="dense"):
    """The bytes of the tape a training forward fills (it holds L, q | k | v, O and everything else the backward reads), on zero-filled
    buffers: hificar_xfmr_forward_train, _ragged or _packed in the model's current arithmetic."""
    lib, h = m._lib, m._handle
    B, _, T = x.shape
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = owned_floats((B, m._params["out_channels"], T), 0x00)
    stats = owned_floats((len(m._batch_norms()), 2, m._params["hidden_dim"]), 0x00)
    if form == "dense":
        ws, ws_ptr, ws_bytes = owned(lib.hificar_xfmr_train_workspace_bytes(h, B, T), 0x00)
        tape, tape_ptr, tape_bytes = owned(lib.hificar_xfmr_tape_bytes(h, B, T), 0x00)
        _native.check(lib.hificar_xfmr_forward_train(h, x.data_ptr(), out.data_ptr(), stats.data_ptr(), B, T, float(p), 4242, 3, tape_ptr, tape_bytes, ws_ptr,
                                                     ws_bytes, stream), "hificar_xfmr_forward_train")
    else:
        host = torch.tensor(list(lengths), dtype=torch.int32)
        on_dev = host.to("cuda:0")
        if form == "ragged":
            ws, ws_ptr, ws_bytes = owned(lib.hificar_xfmr_train_workspace_bytes(h, B, T), 0x00)
            tape, tape_ptr, tape_bytes = owned(lib.hificar_xfmr_tape_bytes(h, B, T), 0x00)
            fwd = lib.hificar_xfmr_forward_train_ragged
        else:
            mp = lib.hificar_xfmr_packed_rows(B, T, host.data_ptr())
            ws, ws_ptr, ws_bytes = owned(lib.hificar_xfmr_train_workspace_bytes_packed(h, B, mp), 0x00)
            tape, tape_ptr, tape_bytes = owned(lib.hificar_xfmr_tape_bytes_packed(h, B, mp), 0x00)
            fwd = lib.hificar_xfmr_forward_train_packed
        _native.check(fwd(h, x.data_ptr(), on_dev.data_ptr(), host.data_ptr(), out.data_ptr(), stats.data_ptr(), B, T, float(p), 4242, 3, tape_ptr, tape_bytes,
                          ws_ptr, ws_bytes, stream), "the ragged training forward")
    torch.cuda.synchronize()
    off = tape_ptr - tape.data_ptr()
    return out, tape[off:off + tape_bytes].clone()


def assert_same_tape(m, x, p, what, lengths=None, form="dense"):
    """One handle, the same forward in bf16x3wac and in bf16x3wack: out and the whole tape (L among it) byte for byte."""
    m._native_handle(train=True)
    m.set_train_precision("bf16x3wac")
    out_c, tape_c = tape_after_forward(m, x, p, lengths, form)
    m.set_train_precision("bf16x3wack")
    out_k, tape_k = tape_after_forward(m, x, p, lengths, form)
    assert tape_k.numel() == tape_c.numel() > 256 and bool(tape_k.any()), what
    assert torch.equal(out_k, out_c) and torch.equal(tape_k, tape_c), what


def same(a, b, m, what):
    """(out, statistics, gradient buffer, dx) of two runs of the C entry points, bit for bit and finite."""
    for q, u, v in zip(("out", "batch statistics", None, "dx"), a, b):
        if q is not None:
            assert torch.isfinite(v).all() and torch.equal(u, v), (what, q)
    for key, off, num in _grad_layout(m):
        assert torch.isfinite(b[2][off:off + num]).all() and torch.equal(a[2][off:off + num], b[2][off:off + num]), (what, key)


def run(name):
    """One bf16x3wack step of a dense case, the float64 reference on its ReLU sides, a second model's step with its profile, and the bf16x3wac
    step of the same model and seed with its profile: computed once per module and left unchanged."""
    if name not in _RUNS:
        params, sd, x, t, shapes = case(name)
        mk = model(params, sd, "bf16x3wack")
        gates = {}
        got = step(mk, x, t, gates=gates)
        ref = O.restatement(name, torch.float64, gates=gates, shapes=shapes)
        mk2 = model(params, sd, "bf16x3wack")
        again, rows_k = profiled(mk2, lambda: step(mk2, x, t))
        mc = model(params, sd, "bf16x3wac")
        x3wac, rows_c = profiled(mc, lambda: step(mc, x, t))
        _RUNS[name] = dict(got=got, ref=ref, again=again, rows_k=rows_k, x3wac=x3wac, rows_c=rows_c)
    return _RUNS[name]


# ------------------------------------------------------------------------------------------------ the dense cases
@pytest.mark.parametrize("name", EK.ALL_DENSE)
def test_profile_rows_by_name_both_ways(name):
    r = run(name)
    print("  " + "\n  ".join(sorted(k for k in r["rows_k"] if "attn" in k or "demb" in k)))
    check_rows(name, r["rows_k"], r["rows_c"], case(name)[0]["elayers"])


@pytest.mark.parametrize("name", EK.ALL_DENSE)
def test_step_against_the_restatement(name):
    r = run(name)
    got, ref = r["got"], r["ref"]
    print(f"  {name}: {ref['gate_flips']} ReLU(s) on the other side than float64's own, the farthest {ref['gate_gap']:.3g} of max |x| from zero")
    assert ref["gate_gap"] < E.X3_OUT_BAR
    assert set(got["grads"]) == set(ref["grads"])
    errs = EK.errors_x3wack(got, ref)
    last = f"grad.transformer.layers.{case(name)[0]['elayers'] - 1}."
    print("  what the new kernels feed first: %s" % ", ".join(f"{t} {errs[last + t][0]:.3g}" for t in MOVED))
    assert_within(errs, name)
    assert torch.isfinite(got["out"]).all() and torch.isfinite(got["dx"]).all()
    assert "libhificar.so" in open("/proc/self/maps").read()


@pytest.mark.parametrize("name", EK.ALL_DENSE)
def test_out_tape_and_dq_are_bitwise_the_bf16x3wac_steps_and_repeats_are_bit_identical(name):
    r = run(name)
    params, sd, x, _, _ = case(name)
    assert_bitwise_up_to_the_key_tiled_kernels(r["got"], r["x3wac"], r["ref"], params, name)
    assert_equal_steps(r["got"], r["again"], name + " on a second model")  # (with and without the debug taps)
    assert_same_tape(model(params, sd, "bf16x3wack"), dev(x), params["dropout"], name)


@pytest.mark.parametrize("name", ["t65", "d48", "d128"])
def test_dirty_scratch_around_a_step_of_another_shape(name):
    params, sd, x, _, _ = case(name)
    B, _, T = x.shape
    p, seed = params["dropout"], O.SEEDS[name]
    m = model(params, sd, "bf16x3wack")
    m._native_handle(train=True)
    xd = dev(x)
    dout = dev(uniform(seed, "dout", (B, params["out_channels"], T), -1.0, 1.0))
    first = native_step(m, xd, dout, p, 0xFF)
    T2 = T - 7  # (another tile count or another ragged last tile; other buffers, the same handle)
    native_step(m, xd[:, :, :T2].contiguous(), dout[:, :, :T2].contiguous(), p, 0xFF)
    same(first, native_step(m, xd, dout, p, 0x00), m, "after a step of another shape, zero-filled buffers")
    same(first, native_step(m, xd, dout, p, 0xFF, lengths=[T] * B), m, "every length = T")
    assert float(first[3].abs().max()) > 0


def test_the_switches_give_fresh_models_steps_and_rebuild_nothing():
    name = "t65"
    params, sd, x, t, _ = case(name)
    m = model(params, sd, "bf16x3wack")
    assert_equal_steps(step(m, x, t), run(name)["got"], name)
    fresh = {"bf16x3wac": lambda: run(name)["x3wac"], "bf16x3wack": lambda: run(name)["got"]}
    for arithmetic in ("bf16x3wac", "bf16x3wa", "bf16x3w", "bf16x3", "f32", "bf16x3wack"):
        m.set_train_precision(arithmetic)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)  # (the running statistics moved)
        m.set_dropout_seed(O.DROPOUT_SEED)
        want = fresh.get(arithmetic, lambda: step(model(params, sd, arithmetic), x, t))()
        assert_equal_steps(step(m, x, t), want, f"{name} after set_train_precision({arithmetic})")
    # bf16x3wac -> bf16x3wack on a handle that has its parameters: no weight pack, no table
    mc = model(params, sd, "bf16x3wac")
    step(mc, x, t)
    mc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    mc.set_dropout_seed(O.DROPOUT_SEED)
    mc._native_handle(train=True)  # (the hand-over of the reloaded parameters, in bf16x3wac: the tables are split here)
    _, rows = profiled(mc, lambda: mc.set_train_precision("bf16x3wack"))
    assert rows == {}, rows
    assert_equal_steps(step(mc, x, t), run(name)["got"], "bf16x3wac -> bf16x3wack")
    # from bf16x3w the tables are split, as towards bf16x3wa
    mw = model(params, sd, "bf16x3w")
    step(mw, x, t)
    mw.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    mw.set_dropout_seed(O.DROPOUT_SEED)
    mw._native_handle(train=True)
    _, rows = profiled(mw, lambda: mw.set_train_precision("bf16x3wack"))
    assert rows == {"xfmr_split_tab_kernel": params["elayers"]}, rows
    assert_equal_steps(step(mw, x, t), run(name)["got"], "bf16x3w -> bf16x3wack")


def test_a_backward_after_a_switch_is_refused_and_the_tape_survives():
    name = "t65"
    params, sd, x, t, _ = case(name)
    straight = run(name)["got"]
    m = model(params, sd, "bf16x3wack")
    xt = dev(x).requires_grad_(True)
    loss = F.l1_loss(m(xt), dev(t))
    for other in ("bf16x3wac", "bf16x3wa", "f32"):
        m.set_train_precision(other)
        with pytest.raises(RuntimeError, match=f"training arithmetic is {other}, its last training forward ran in bf16x3wack"):
            loss.backward(retain_graph=True)
        assert xt.grad is None and all(q.grad is None for q in m.parameters())
    m.set_train_precision("bf16x3wack")
    loss.backward()
    assert torch.equal(xt.grad, straight["dx"]) and all(torch.equal(q.grad, straight["grads"][k]) for k, q in m.named_parameters())


def test_workspace_and_tape_are_those_of_bf16x3wac():
    params, sd, _, _, _ = case("t65")
    m = model(params, sd, "bf16x3wac")
    m._native_handle(train=True)
    lib, h = m._lib, m._handle
    host = torch.tensor([70, 33, 1], dtype=torch.int32)
    mp = lib.hificar_xfmr_packed_rows(3, 70, host.data_ptr())
    sizes = lambda: (lib.hificar_xfmr_train_workspace_bytes(h, 2, 65), lib.hificar_xfmr_train_workspace_bytes_packed(h, 3, mp),  # noqa: E731
                     lib.hificar_xfmr_train_workspace_bytes(h, 16, 257), lib.hificar_xfmr_tape_bytes(h, 2, 65), lib.hificar_xfmr_tape_bytes_packed(h, 3, mp))
    x3wac = sizes()
    m.set_train_precision("bf16x3wack")
    assert sizes() == x3wac and all(x3wac)  # the bands are read as bf16x3wac leaves them: no copy, no scratch of this arithmetic's own


# ------------------------------------------------------------------------------------------------ the ragged batches, padded and packed
def ragged_model(name, arithmetic):
    params, sd, x, t, lengths = R.ragged_case(name)
    return model(params, sd, arithmetic), params, x, t, lengths


@pytest.mark.parametrize("form", ["ragged", "packed"])
@pytest.mark.parametrize("name", EK.RAGGED_CASES)
def test_ragged_and_packed_steps(name, form):
    m, params, x, t, lengths = ragged_model(name, "bf16x3wack")
    gates = {}
    got = pstep(m, x, t, lengths, form=form, gates=gates)
    ref = R.ragged_restatement(name, torch.float64, gates=gates)
    print(f"  {name} {form}: {ref['gate_flips']} ReLU(s) on the other side than float64's own, the farthest {ref['gate_gap']:.3g} of max |x| from zero")
    assert ref["gate_gap"] < E.X3_OUT_BAR
    assert_within(EK.errors_x3wack(got, ref), f"{name} {form}")
    assert float(padded(got["out"], lengths).abs().max()) == 0.0 and float(padded(got["dx"], lengths).abs().max()) == 0.0
    mk, mc = ragged_model(name, "bf16x3wack")[0], ragged_model(name, "bf16x3wac")[0]
    again, rows_k = profiled(mk, lambda: pstep(mk, x, t, lengths, form=form))
    x3wac, rows_c = profiled(mc, lambda: pstep(mc, x, t, lengths, form=form))
    check_rows(f"{name} {form}", rows_k, rows_c, params["elayers"])
    assert_equal_steps(got, again, f"{name} {form} on a second model")
    assert_bitwise_up_to_the_key_tiled_kernels(got, x3wac, ref, params, f"{name} {form}")
    assert_same_tape(mk, dev(x), params["dropout"], f"{name} {form}", lengths, form)


def test_nan_on_padded_frames_changes_nothing_padded_and_packed():
    name = "mixed"
    m, params, x, _, lengths = ragged_model(name, "bf16x3wack")
    m._native_handle(train=True)
    B, _, T = x.shape
    p, seed = params["dropout"], R.RAGGED_SEEDS[name]
    x = dev(x)
    dout = dev(uniform(seed, "dout", (B, params["out_channels"], T), -1.0, 1.0))
    dense = native_step(m, x, dout, p, 0x00)
    # zeros on padded frames; NaN there in x and dout, on 0xFF-filled buffers, gives the same bits: rows past a length and gap rows are never
    # read as data by the new kernels (the staging writes zeros for them, a band entry is read only where it was written), and the padded
    # keys' own dk | dv rows come out as zeros
    pad = (~R.valid_mask(lengths, T)).to("cuda:0")[:, None, :]
    xz, dz = x.masked_fill(pad, 0.0).contiguous(), dout.masked_fill(pad, 0.0).contiguous()
    xn, dn = x.masked_fill(pad, float("nan")).contiguous(), dout.masked_fill(pad, float("nan")).contiguous()
    for what, fn in (("ragged", lambda *a: native_step(m, *a, lengths=lengths)), ("packed", lambda *a: native_packed_step(m, *a, lengths))):
        clean, dirty = fn(xz, dz, p, 0x00), fn(xn, dn, p, 0xFF)
        same(clean, dirty, m, what)
        assert float(padded(dirty[0], lengths).abs().max()) == 0.0 and float(padded(dirty[3], lengths).abs().max()) == 0.0, what
        assert not torch.equal(clean[0], dense[0])


# ------------------------------------------------------------------------------------------------ five steps through the trainer
def test_five_steps_through_the_trainer_then_back_to_bf16x3wac():
    params, sd, _, _ = O.case(O.STEPS_CASE)
    tr = InversionTrainer(dict(steps_config(params), train_precision="bf16x3wack"), torch.device("cuda:0"))
    tr.G.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    tr.G.set_dropout_seed(O.DROPOUT_SEED)
    assert tr.G.train_precision == "bf16x3wack" and tr.optimizer["generator"].defaults.get("fused") is True
    losses = [float(tr.train_step(batch_of(s))["train/generator_loss"]) for s in range(O.STEPS["n"])]
    ref_losses, ref_final = O.five_steps(torch.float64)
    e_loss, worst = O.five_step_errors(losses, dict(tr.G.state_dict()), ref_losses, ref_final)
    print("losses", losses, "deviation", e_loss, "worst final tensor", max(worst, key=worst.get), max(worst.values()))
    assert e_loss < EK.BARS_X3WACK["steps_loss"]
    assert max(worst.values()) < EK.BARS_X3WACK["steps_params"]
    # back to bf16x3wac on the same handle: the next step is a fresh bf16x3wac model's on the same state_dict, bitwise
    tr.G.set_train_precision("bf16x3wac")
    fresh = Transformer(train_precision="bf16x3wac", **params)
    fresh.load_state_dict(tr.G.state_dict(), strict=True)
    fresh = fresh.to("cuda:0").train()
    fresh.set_dropout_seed(O.DROPOUT_SEED, offset=tr.G._calls)
    _, _, x, t = O.case(O.STEPS_CASE, 7)
    assert_equal_steps(step(tr.G, x, t), step(fresh, x, t), "after five bf16x3wack steps")
