"""The Transformer's opt-in bf16x3 training arithmetic on a MI355X (``train_precision="bf16x3"``: every forward GEMM and every data gradient
of the training step in the conv engine's bf16x3 kernels; weight gradients, attention, norms, dropout and the tape in fp32), against the
float64 restatement on the device's own ReLU sides and the golden vectors of the real class.  ``pytest -m gpu``.

Bars: transformer_train_bf16x3_emulation.BARS_X3, set on the CPU before the first GPU run (tests/test_transformer_train_bf16x3_host.py holds
the emulation to a quarter of them).  A ReLU may be taken on another side than float64 takes it only where float64's input lies within the
bf16x3 output bar (2e-4, relative) of zero.
"""

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import transformer_ragged_oracle as R
import transformer_train_bf16x3_emulation as E
import transformer_train_oracle as O
from conftest import GOLDEN
from test_gpu_transformer_packed import native_packed_step, pstep
from test_gpu_transformer_ragged import native_step, padded
from test_gpu_transformer_train import assert_within, batch_of, build, dev, step, steps_config
from test_transformer_train_bf16x3_host import device_pack
from test_transformer_train_host import golden_errors
from articulatory_amd import _native
from articulatory_amd.bin.train import InversionTrainer
from articulatory_amd.models import Transformer
from articulatory_amd.models.transformer import _grad_layout
from articulatory_amd.utils.synth import uniform

pytestmark = pytest.mark.gpu


def build_x3(name, arithmetic="bf16x3"):
    m, x, t = build(name)
    m.set_train_precision(arithmetic)
    return m, x, t


def reference(name, gates):
    ref = O.restatement(name, torch.float64, gates=gates)
    print(f"  {name}: {ref['gate_flips']} ReLU(s) on the other side than float64's own, the farthest {ref['gate_gap']:.3g} of max |x| from zero")
    assert ref["gate_gap"] < E.X3_OUT_BAR
    return ref


def profiled(m, fn):
    """{kernel name: launches} of what ``fn`` launches on the model's engine."""
    eng = m.engine()  # (first: it is what loads m._lib)
    lib = m._lib
    _native.check(lib.hificar_profile_begin(eng), "hificar_profile_begin")
    out = fn()
    return out, {r["name"]: r["launches"] for r in _native.profile_rows(lib, eng, 128)[0]}


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", E.CASES)
def test_step_against_the_restatement(name):
    m, x, t = build_x3(name)
    gates = {}
    got = step(m, x, t, gates=gates)
    ref = reference(name, gates)
    assert set(got["grads"]) == set(ref["grads"])
    assert_within(E.errors_x3(got, ref), name)
    assert torch.isfinite(got["out"]).all() and torch.isfinite(got["dx"]).all()
    if name != O.GOLD_CASE:
        return
    # ... and against the real class (dropout 0; its tables get no gradient there: golden_errors skips them), the stored gradients moved by
    # what the device's gates change in the float64 restatement (tests/test_gpu_transformer_train.py: test_golden_case_of_the_reference_class)
    gold = np.load(os.path.join(GOLDEN, "gold_transformer_train.npz"))
    got["grads"] = {k: g.cpu().double() for k, g in got["grads"].items()}
    got["dx"] = got["dx"].cpu().double()
    if ref["gate_flips"]:
        own = O.restatement(name, torch.float64)
        got["dx"] = got["dx"] - (ref["dx"] - own["dx"])
        got["grads"] = {k: g - (ref["grads"][k] - own["grads"][k]) for k, g in got["grads"].items()}
    assert_within({k: (e, E.BARS_X3[k.split(".")[0]]) for k, (e, _) in golden_errors(gold, name, got).items()}, "golden")


# ------------------------------------------------------------------------------------------------ 2, 3
def test_the_arithmetic_runs_where_it_is_asked_for_and_nowhere_else():
    name = "t65"
    m3, x, t = build_x3(name)
    a, k3 = profiled(m3, lambda: step(m3, x, t))
    print("  bf16x3 step:", k3)
    assert not any(k.startswith(("conv_f32do_kernel", "conv_sk_")) for k in k3)
    assert any(k.startswith("conv_bf16x3") for k in k3) and k3.get("xfmr_split_rows_kernel", 0) > 0 and k3.get("pack16_kernel", 0) > 0
    assert any(k.startswith("wgrad_") for k in k3) and "xfmr_attn_kernel<train>" in k3 and "xfmr_attn_bwd_kernels" in k3
    m1, _, _ = build(name)  # no keyword
    b, k1 = profiled(m1, lambda: step(m1, x, t))
    assert any(k.startswith("conv_f32do_kernel") for k in k1)
    assert not any(k.startswith("conv_bf16x3") or k in ("xfmr_split_rows_kernel", "pack16_kernel") for k in k1)
    assert {k: v for k, v in k1.items() if k.startswith(("wgrad_", "wreduce_", "xfmr_attn"))} == {k: v for k, v in k3.items() if k.startswith(("wgrad_", "wreduce_", "xfmr_attn"))}
    # the two arithmetics differ, and agree within the bar
    assert not torch.equal(a["out"], b["out"])
    assert float((a["out"] - b["out"]).abs().max() / b["out"].abs().max()) < E.BARS_X3["out"]
    # train_precision="f32", by keyword or by the setter on a model that was bf16x3, is the model built without the keyword, bitwise
    params, sd, _, _ = O.case(name)
    m2 = Transformer(train_precision="f32", **params)
    m2.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m2 = m2.to("cuda:0").train()
    m2.set_dropout_seed(O.DROPOUT_SEED)
    m4, _, _ = build_x3(name)
    step(m4, x, t)
    m4.set_train_precision("f32")
    m4.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)  # (the running statistics moved)
    m4.set_dropout_seed(O.DROPOUT_SEED)
    for other in (step(m2, x, t), step(m4, x, t)):
        assert torch.equal(other["out"], b["out"]) and torch.equal(other["dx"], b["dx"]) and torch.equal(other["stats"], b["stats"])
        assert all(torch.equal(other["grads"][k], g) for k, g in b["grads"].items())
    # the eval forward of a bf16x3-training model — on the handle that trained — is the exact-fp32 eval forward of its parameters and
    # running statistics: what a fresh fp32 model computes from the same state_dict
    y3, ke = profiled(m3, lambda: m3.eval()(dev(x)))
    assert m3.train_precision == "bf16x3" and any(k.startswith("conv_f32do_kernel") for k in ke) and not any(k.startswith("conv_bf16x3") for k in ke)
    fresh = Transformer(**params)
    fresh.load_state_dict(m3.state_dict(), strict=True)
    assert torch.equal(fresh.eval().to("cuda:0")(dev(x)), y3)


# ------------------------------------------------------------------------------------------------ 4, 5
def ragged_model(arithmetic="bf16x3"):
    params, sd, x, t, lengths = R.ragged_case(E.RAGGED_CASE)
    m = Transformer(train_precision=arithmetic, **params)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to("cuda:0").train()
    m.set_dropout_seed(O.DROPOUT_SEED)
    return m, params, x, t, lengths


def same(a, b, m, what):
    for q, u, v in zip(("out", "batch statistics", None, "dx"), a, b):
        if q is not None:
            assert torch.isfinite(v).all() and torch.equal(u, v), (what, q)
    for key, off, num in _grad_layout(m):
        assert torch.isfinite(b[2][off:off + num]).all() and torch.equal(a[2][off:off + num], b[2][off:off + num]), (what, key)


def test_ragged_and_packed_forms_padded_frames_and_dirty_scratch():
    m, params, x, _, lengths = ragged_model()
    m._native_handle(train=True)
    B, _, T = x.shape
    p, seed = params["dropout"], R.RAGGED_SEEDS[E.RAGGED_CASE]
    x = dev(x)
    dout = dev(uniform(seed, "dout", (B, params["out_channels"], T), -1.0, 1.0))
    # every length = T: the dense bf16x3 step, bitwise; and what tape, workspace and outputs hold on entry does not matter (dense form)
    dense = native_step(m, x, dout, p, 0x00)
    same(dense, native_step(m, x, dout, p, 0xFF), m, "dense on 0xFF-filled buffers")
    same(dense, native_step(m, x, dout, p, 0x00, lengths=[T] * B), m, "every length = T")
    assert float(dense[3].abs().max()) > 0
    # the ragged and the packed step: zeros on padded frames; NaN there in x and dout, on 0xFF-filled buffers, changes nothing
    pad = (~R.valid_mask(lengths, T)).to("cuda:0")[:, None, :]
    xz, dz = x.masked_fill(pad, 0.0).contiguous(), dout.masked_fill(pad, 0.0).contiguous()
    xn, dn = x.masked_fill(pad, float("nan")).contiguous(), dout.masked_fill(pad, float("nan")).contiguous()
    for what, fn in (("ragged", lambda *a: native_step(m, *a, lengths=lengths)), ("packed", lambda *a: native_packed_step(m, *a, lengths))):
        clean, dirty = fn(xz, dz, p, 0x00), fn(xn, dn, p, 0xFF)
        same(clean, dirty, m, what)
        assert float(padded(dirty[0], lengths).abs().max()) == 0.0 and float(padded(dirty[3], lengths).abs().max()) == 0.0, what
        assert not torch.equal(clean[0], dense[0])


@pytest.mark.parametrize("form", ["ragged", "packed"])
def test_ragged_and_packed_steps_against_the_ragged_restatement(form):
    m, params, x, t, lengths = ragged_model()
    gates = {}
    got = pstep(m, x, t, lengths, form=form, gates=gates)
    ref = R.ragged_restatement(E.RAGGED_CASE, torch.float64, gates=gates)
    print(f"  {form}: {ref['gate_flips']} ReLU(s) on the other side than float64's own, the farthest {ref['gate_gap']:.3g} of max |x| from zero")
    assert ref["gate_gap"] < E.X3_OUT_BAR
    assert_within(E.errors_x3(got, ref), form)
    _, kernels = profiled(m, lambda: pstep(m, x, t, lengths, form=form))
    assert any(k.startswith("conv_bf16x3") for k in kernels) and not any(k.startswith("conv_f32do_kernel") for k in kernels)


def test_workspace_grows_by_the_split_rows_and_the_tape_does_not():
    m, _, _ = build_x3("t65", "f32")
    m._native_handle(train=True)
    lib, h = m._lib, m._handle
    host = torch.tensor([70, 33, 1], dtype=torch.int32)
    mp = lib.hificar_xfmr_packed_rows(3, 70, host.data_ptr())
    f32 = (lib.hificar_xfmr_train_workspace_bytes(h, 2, 65), lib.hificar_xfmr_train_workspace_bytes_packed(h, 3, mp))
    tapes = (lib.hificar_xfmr_tape_bytes(h, 2, 65), lib.hificar_xfmr_tape_bytes_packed(h, 3, mp))
    m.set_train_precision("bf16x3")
    x3 = (lib.hificar_xfmr_train_workspace_bytes(h, 2, 65), lib.hificar_xfmr_train_workspace_bytes_packed(h, 3, mp))
    # one buffer of split rows, 3072 columns of 4 bytes: B T + 64 rounded up to 256 rows, or the packed rows
    assert x3[0] - f32[0] == 256 * 3072 * 4 and x3[1] - f32[1] == mp * 3072 * 4
    assert tapes == (lib.hificar_xfmr_tape_bytes(h, 2, 65), lib.hificar_xfmr_tape_bytes_packed(h, 3, mp))
    m.set_train_precision("f32")
    assert f32 == (lib.hificar_xfmr_train_workspace_bytes(h, 2, 65), lib.hificar_xfmr_train_workspace_bytes_packed(h, 3, mp))


# ------------------------------------------------------------------------------------------------ 6
def test_five_steps_through_the_trainer_then_back_to_f32():
    params, sd, _, _ = O.case(O.STEPS_CASE)
    tr = InversionTrainer(dict(steps_config(params), train_precision="bf16x3"), torch.device("cuda:0"))
    tr.G.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    tr.G.set_dropout_seed(O.DROPOUT_SEED)
    assert tr.G.train_precision == "bf16x3" and tr.optimizer["generator"].defaults.get("fused") is True
    losses = [float(tr.train_step(batch_of(s))["train/generator_loss"]) for s in range(O.STEPS["n"])]
    ref_losses, ref_final = O.five_steps(torch.float64)
    e_loss, worst = O.five_step_errors(losses, dict(tr.G.state_dict()), ref_losses, ref_final)
    print("losses", losses, "deviation", e_loss, "worst final tensor", max(worst, key=worst.get), max(worst.values()))
    assert e_loss < E.BARS_X3["steps_loss"]
    assert max(worst.values()) < E.BARS_X3["steps_params"]
    # back to fp32 on the same handle: the next step is a fresh fp32 model's on the same state_dict, bitwise
    tr.G.set_train_precision("f32")
    fresh = Transformer(**params)
    fresh.load_state_dict(tr.G.state_dict(), strict=True)
    fresh = fresh.to("cuda:0").train()
    fresh.set_dropout_seed(O.DROPOUT_SEED, offset=tr.G._calls)
    _, _, x, t = O.case(O.STEPS_CASE, 7)
    a, b = step(tr.G, x, t), step(fresh, x, t)
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["dx"], b["dx"]) and torch.equal(a["stats"], b["stats"])
    assert all(torch.equal(a["grads"][k], g) for k, g in b["grads"].items())


# ------------------------------------------------------------------------------------------------ 7
def test_a_backward_in_the_other_arithmetic_is_refused_and_the_tape_survives():
    m, x, t = build_x3("t65")
    straight = step(m, x, t)
    m2, _, _ = build_x3("t65")
    xt = dev(x).requires_grad_(True)
    loss = F.l1_loss(m2(xt), dev(t))
    m2.set_train_precision("f32")
    with pytest.raises(RuntimeError, match="training arithmetic is f32, its last training forward ran in bf16x3"):
        loss.backward(retain_graph=True)
    assert xt.grad is None and all(p.grad is None for p in m2.parameters())
    m2.set_train_precision("bf16x3")
    loss.backward()
    assert torch.equal(xt.grad, straight["dx"])
    assert all(torch.equal(p.grad, straight["grads"][k]) for k, p in m2.named_parameters())


# ------------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("cout,cin,cin_pad,K", [(128, 12, 32, 3), (384, 128, 128, 1), (40, 128, 128, 1), (3072, 768, 768, 1), (768, 768, 768, 3)])
@pytest.mark.parametrize("mode", [0, 2])
def test_device_pack_bytes_are_the_host_packs(cout, cin, cin_pad, K, mode):
    """pack16_kernel over a buffer of 0xFF bytes against pack_w16, the pack of the inference handles, read back; and against the kernel's
    index functions run on the host (what tests/test_transformer_train_bf16x3_host.py holds to the layout's definition)."""
    w = uniform(9200 + cout + cin + K, "pack", (cout, cin, K), -1.0, 1.0)
    on_device, on_host, want = device_pack(w, cin_pad, mode, 1), device_pack(w, cin_pad, mode, 0), device_pack(w, cin_pad, mode, 2)
    assert np.array_equal(on_device, want) and np.array_equal(on_host, want)
    assert len(np.unique(want)) > 100
