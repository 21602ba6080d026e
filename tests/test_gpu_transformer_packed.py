"""Packed Transformer training on a MI355X: ``Transformer.forward_padded(packed=True)`` + ``masked_l1_loss`` through
``hificar_xfmr_forward_train_packed`` / ``hificar_xfmr_backward_packed`` against the float64 restatement of the ragged step
(tests/transformer_ragged_oracle.py: the packed step computes the same function), against the ragged and the dense device steps, bitwise
independence of whatever padded frames and scratch hold, the tape's size, eval after a step, the trainer's ``pad_packed`` and the refusals.
Shapes: tests/transformer_packed_shapes.py; bars: transformer_train_oracle.BARS.  ``pytest -m gpu``.
"""

import ctypes

import numpy as np
import pytest
import torch

import transformer_packed_shapes as P
import transformer_ragged_oracle as R
import transformer_train_oracle as O
from conftest import rel_err
from test_gpu_bigru_train_edges import owned, owned_floats
from test_gpu_transformer_ragged import build, native_step, pad_batch, pad_config, padded
from test_gpu_transformer_train import assert_within, dev
from transformer_oracle import TransformerOracle
from articulatory_amd import _native
from articulatory_amd.bin.train import InversionTrainer
from articulatory_amd.losses import masked_l1_loss
from articulatory_amd.models.transformer import _grad_layout
from articulatory_amd.utils.synth import uniform

pytestmark = pytest.mark.gpu
E_INVALID, E_STATE, E_WORKSPACE = -1, -2, -4  # include/hificar.h


def pstep(m, x, t, lengths, form="packed", need_dx=True, gates=None):
    """One forward + masked L1 + backward on the device in the restatement's result layout; form: "packed", "ragged" (forward_padded) or
    "dense" (forward; every length = T).  ``gates``: receives which side of every ReLU the device took, from the debug taps, which a packed
    forward delivers in the padded (B, T, width) layout with zeros on padded frames."""
    for p in m.parameters():
        p.grad = None
    xt = dev(x).requires_grad_(need_dx)
    bufs = {}
    if gates is not None:
        B, _, T = x.shape
        m._native_handle(train=True)
        for name in O.relu_names(m._params):
            bufs[name] = torch.full((B, T, 3072 if name.endswith("hidden") else m._params["hidden_dim"]), float("nan"), dtype=torch.float32, device="cuda:0")
            m.debug_tap(name, bufs[name])
    y = m(xt) if form == "dense" else m.forward_padded(xt, lengths, packed=form == "packed")
    if gates is not None:
        m.debug_tap(None)
        pad = (~R.valid_mask(lengths, x.shape[2])).to("cuda:0")
        for name, buf in bufs.items():
            assert torch.isfinite(buf).all() and float(buf[pad].abs().max() if bool(pad.any()) else 0.0) == 0.0, name
            gates[name] = (buf > 0).cpu() if name.endswith("hidden") else (buf > 0).transpose(1, 2).cpu()
    loss = masked_l1_loss(y, dev(t), lengths)
    loss.backward()
    return dict(out=y.detach(), loss=loss.detach(), dx=xt.grad, grads={k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None},
                stats=m._last_stats.clone(), running={k: v.detach().clone() for k, v in m.named_buffers() if k.endswith(("running_mean", "running_var"))})


def assert_zero_on_padding(got, lengths, T):
    if sum(lengths) < len(lengths) * T:
        assert float(padded(got["out"], lengths).abs().max()) == 0.0 and float(padded(got["dx"], lengths).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", list(P.ALL_SHAPES))
def test_packed_shape_against_float64_restatement(name):
    params, sd, x, t, lengths = P.packed_case(name)
    m = build(params, sd)
    before = [int(bn.num_batches_tracked) for bn in m._batch_norms()]
    gates = {}
    got = pstep(m, x, t, lengths, gates=gates)
    ref = P.packed_restatement(name, torch.float64, gates=gates)
    print(f"  {name}: {ref['gate_flips']} ReLU(s) on the other side than float64's own, the farthest {ref['gate_gap']:.3g} of max |x| from zero")
    assert ref["gate_gap"] < O.GATE_GAP
    assert set(got["grads"]) == set(ref["grads"])
    assert_within(O.errors(got, ref), name)  # (prints the five largest shares of a bar)
    assert torch.isfinite(got["out"]).all() and torch.isfinite(got["dx"]).all()
    assert_zero_on_padding(got, lengths, x.shape[2])
    assert [int(bn.num_batches_tracked) for bn in m._batch_norms()] == [n + 1 for n in before] and m._calls == 1
    assert "libhificar.so" in open("/proc/self/maps").read()


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("name", ["tiles", "chunks", "many", "edge256"])
def test_packed_against_the_ragged_device_step(name):
    """The same model, inputs and seed through both forms: the masks are equal (dropout elements are those of the padded tensors), so the
    two steps differ by the order of their sums over rows only — which is what lets this hold at p = 0.5 (`tiles`)."""
    params, sd, x, t, lengths = P.packed_case(name)
    ragged = pstep(build(params, sd), x, t, lengths, form="ragged")
    packed = pstep(build(params, sd), x, t, lengths, form="packed")
    errs = O.errors(packed, ragged)
    k = max(errs, key=lambda q: errs[q][0] / errs[q][1])
    print(f"  {name} (p = {params['dropout']}): packed against ragged, the largest share of a bar: {k} {errs[k][0] / errs[k][1]:.3g}")
    assert_within(errs, name)
    assert_zero_on_padding(packed, lengths, x.shape[2])


# ------------------------------------------------------------------------------------------------ 3
def test_all_lengths_full_against_the_dense_step():
    """`mixed`'s model at B = 2, T = 65, nothing padded: within the bars of the dense step, not bitwise (256-row chunks of packed rows, and
    one run of Mp rows per GEMM)."""
    params, sd, _, _, _ = P.packed_case("mixed")
    seed, B, T = P.seed_of("mixed"), 2, 65
    x = uniform(seed, "full.x", (B, params["in_channels"], T), -1.0, 1.0)
    t = uniform(seed, "full.t", (B, params["out_channels"], T), 4.0, 5.0)
    dense = pstep(build(params, sd), x, t, (T,) * B, form="dense")
    packed = pstep(build(params, sd), x, t, (T,) * B, form="packed")
    assert_within(O.errors(packed, dense), "all lengths = T")


# ------------------------------------------------------------------------------------------------ the C entry points on owned buffers
def lens_pair(lengths):
    host = torch.tensor(list(lengths), dtype=torch.int32)
    return host, host.to("cuda:0")


def native_packed_step(m, x, dout, p, fill, lengths, with_tape=True, more_ws=0):
    """hificar_xfmr_forward_train_packed, then hificar_xfmr_backward_packed with a tape; every scratch and output buffer pre-filled with
    ``fill`` bytes, the workspace ``more_ws`` bytes larger than asked for: (out, batch statistics, grads, dx)."""
    lib, h = m._lib, m._handle
    B, C, T = x.shape
    host, on_dev = lens_pair(lengths)
    mp = lib.hificar_xfmr_packed_rows(B, T, host.data_ptr())
    assert mp == P.packed_rows(lengths)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = owned_floats((B, m._params["out_channels"], T), fill)
    stats = owned_floats((len(m._batch_norms()), 2, m._params["hidden_dim"]), fill)
    ws, ws_ptr, ws_bytes = owned(lib.hificar_xfmr_train_workspace_bytes_packed(h, B, mp) + more_ws, fill)
    tape, tape_ptr, tape_bytes = owned(lib.hificar_xfmr_tape_bytes_packed(h, B, mp), fill) if with_tape else (None, None, 0)
    _native.check(lib.hificar_xfmr_forward_train_packed(h, x.data_ptr(), on_dev.data_ptr(), host.data_ptr(), out.data_ptr(), stats.data_ptr(), B, T, float(p),
                                                        4242, 3, tape_ptr, tape_bytes, ws_ptr, ws_bytes, stream), "hificar_xfmr_forward_train_packed")
    if not with_tape:
        torch.cuda.synchronize()
        return out, stats, None, None
    grads = owned_floats((int(lib.hificar_xfmr_grad_floats(h)),), fill)
    dx = owned_floats((B, C, T), fill)
    _native.check(lib.hificar_xfmr_backward_packed(h, dout.data_ptr(), host.data_ptr(), B, T, tape_ptr, tape_bytes, grads.data_ptr(), dx.data_ptr(), ws_ptr,
                                                   ws_bytes, stream), "hificar_xfmr_backward_packed")
    torch.cuda.synchronize()
    return out, stats, grads, dx


def native_model(name):
    params, sd, x, _, lengths = P.packed_case(name)
    m = build(params, sd)
    m._native_handle(train=True)
    dout = dev(uniform(P.seed_of(name), "dout", x.shape[:1] + (params["out_channels"],) + x.shape[2:], -1.0, 1.0))
    return m, params, dev(x), dout, lengths


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("name", ["mixed", "zero", "many", "edge256"])
def test_results_depend_neither_on_padded_frames_nor_on_scratch(name):
    """x and dout zero in the padded frames on zero-filled buffers, against x and dout NaN there on 0xFF-filled buffers (tape, workspace,
    out, statistics, gradient buffer, dx) with a larger workspace: finite and bitwise equal, with and without a tape; and twice the same."""
    m, params, x, dout, lengths = native_model(name)
    pad = (~R.valid_mask(lengths, x.shape[2])).to("cuda:0")[:, None, :]
    assert bool(pad.any())
    p = params["dropout"]
    xz, dz = x.masked_fill(pad, 0.0).contiguous(), dout.masked_fill(pad, 0.0).contiguous()
    xn, dn = x.masked_fill(pad, float("nan")).contiguous(), dout.masked_fill(pad, float("nan")).contiguous()
    clean = native_packed_step(m, xz, dz, p, 0x00, lengths)
    again = native_packed_step(m, xz, dz, p, 0x00, lengths)
    dirty = native_packed_step(m, xn, dn, p, 0xFF, lengths, more_ws=1 << 20)
    assert torch.isnan(owned_floats((4,), 0xFF)).all()
    layout = _grad_layout(m)
    for what, a, b, c in zip(("out", "batch statistics", "grads", "dx"), clean, dirty, again):
        assert torch.isfinite(b).all(), what
        assert torch.equal(a, b) and torch.equal(a, c), what
    assert float(padded(dirty[0], lengths).abs().max()) == 0.0 and float(padded(dirty[3], lengths).abs().max()) == 0.0
    # (a conv bias in front of a batch norm has a mathematically zero gradient: rounding may make it exactly 0)
    assert float(clean[3].abs().max()) > 0 and all(float(clean[2][off:off + num].abs().max()) > 0 for k, off, num in layout
                                                   if not k.endswith(O.STEPS_UNCOMPARED))
    light = native_packed_step(m, xn, dn, p, 0xFF, lengths, with_tape=False)
    assert torch.equal(light[0], clean[0]) and torch.equal(light[1], clean[1])  # the same arithmetic with and without a tape


# ------------------------------------------------------------------------------------------------ 5
def test_the_packed_tape_is_smaller_by_the_padding():
    params, sd, _, _, _ = P.packed_case("mixed")
    m = build(params, sd)
    m._native_handle(train=True)
    lib, h = m._lib, m._handle
    for name in ("chunks", "many"):
        _, B, T, lengths, _ = P.ALL_SHAPES[name]
        packed, dense = lib.hificar_xfmr_tape_bytes_packed(h, B, P.packed_rows(lengths)), lib.hificar_xfmr_tape_bytes(h, B, T)
        print(f"  {name}: tape {packed} bytes packed, {dense} padded")
        assert 0 < packed < dense, name
    # an all-full batch: above the padded tape by no more than the gap and rounding rows (and the two tables)
    B, T = 4, 130
    mp = P.packed_rows((T,) * B)
    packed, dense = lib.hificar_xfmr_tape_bytes_packed(h, B, mp), lib.hificar_xfmr_tape_bytes(h, B, T)
    per_row = dense / (B * T)  # (an upper estimate of a row's bytes: the padded tape has slack rows of its own)
    assert dense < packed <= dense + (mp - B * T + 256) * per_row + 4 * (mp + B + 1) + 512


# ------------------------------------------------------------------------------------------------ 6
def test_eval_after_a_packed_step_is_the_eval_path_on_the_updated_statistics():
    params, sd, x, t, lengths = P.packed_case("mixed")
    m = build(params, sd)
    pstep(m, x, t, lengths)
    o = R.TransformerRaggedOracle(sd, dtype=torch.float64, dropout=params["dropout"], seed=O.DROPOUT_SEED)
    o.step_padded(x, t, lengths)  # the same step: its running statistics (updated with M / (M - 1)) are what eval mode goes by
    assert sum(lengths) != x.shape[0] * x.shape[2]
    for k, v in o.buffers.items():
        assert rel_err(dict(m.named_buffers())[k].cpu().numpy(), v.numpy()) < O.BARS["out"], k
    m.eval()
    with torch.no_grad():
        y = m(dev(x), lengths=list(lengths))
        assert torch.equal(m.forward_padded(dev(x), lengths, packed=True), y)  # eval(): the flag has no effect
    assert float(padded(y, lengths).abs().max()) == 0.0
    ev = TransformerOracle({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()})
    for b, n in enumerate(lengths):
        assert rel_err(y[b:b + 1, :, :n].cpu().numpy(), ev.forward(x[b:b + 1, :, :n]).numpy()) < O.BARS["out"], b


# ------------------------------------------------------------------------------------------------ 7
def test_three_pad_packed_steps_through_the_trainer():
    params, sd, _, _, _ = R.ragged_case(R.STEPS3_CASE)
    tr = InversionTrainer(dict(pad_config(), pad_packed=True), torch.device("cuda:0"))
    assert tr.packed
    tr.G.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    tr.G.set_dropout_seed(O.DROPOUT_SEED)
    before = int(tr.G.conv_blocks[0].bn1.num_batches_tracked)
    losses = [float(tr.train_step(pad_batch(s))["train/generator_loss"]) for s in range(R.STEPS3["n"])]
    ref, _ = R.run_steps3(torch.float64)
    errs = [abs(a - b) / abs(b) for a, b in zip(losses, ref)]
    print("losses", losses, "deviation from the float64 restatement", errs)
    assert max(errs) < R.STEPS3_LOSS_BAR
    assert tr.steps == R.STEPS3["n"] and int(tr.G.conv_blocks[0].bn1.num_batches_tracked) == before + R.STEPS3["n"]


# ------------------------------------------------------------------------------------------------ 8
def test_refusals_on_the_device():
    m, params, x, dout, lengths = native_model("mixed")
    lib, h = m._lib, m._handle
    B, C, T = x.shape
    p = params["dropout"]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    host, on_dev = lens_pair(lengths)
    mp = lib.hificar_xfmr_packed_rows(B, T, host.data_ptr())
    out = owned_floats((B, params["out_channels"], T), 0)
    stats = owned_floats((len(m._batch_norms()), 2, params["hidden_dim"]), 0)
    grads = owned_floats((int(lib.hificar_xfmr_grad_floats(h)),), 0)
    dx = owned_floats((B, C, T), 0)
    wb, tb = lib.hificar_xfmr_train_workspace_bytes_packed(h, B, mp), lib.hificar_xfmr_tape_bytes_packed(h, B, mp)
    wb = max(wb, lib.hificar_xfmr_train_workspace_bytes(h, B, T))  # one workspace and one tape for both kinds of step
    tb_all = max(tb, lib.hificar_xfmr_tape_bytes(h, B, T))
    ws, ws_ptr, _ = owned(wb, 0)
    tape, tape_ptr, _ = owned(tb_all, 0)

    def fwd(host_lens, dev_lens=on_dev, tape_bytes=tb_all, ws_bytes=wb):
        return lib.hificar_xfmr_forward_train_packed(h, x.data_ptr(), dev_lens.data_ptr(), host_lens.data_ptr() if host_lens is not None else None,
                                                     out.data_ptr(), stats.data_ptr(), B, T, p, 1, 0, tape_ptr, tape_bytes, ws_ptr, ws_bytes, stream)

    def bwd(host_lens, tape_bytes=tb_all, ws_bytes=wb):
        return lib.hificar_xfmr_backward_packed(h, dout.data_ptr(), host_lens.data_ptr(), B, T, tape_ptr, tape_bytes, grads.data_ptr(), dx.data_ptr(), ws_ptr,
                                                ws_bytes, stream)

    def bwd_plain():
        return lib.hificar_xfmr_backward(h, dout.data_ptr(), B, T, tape_ptr, tb_all, grads.data_ptr(), dx.data_ptr(), ws_ptr, wb, stream)

    # the forward's own checks, before anything is enqueued
    assert fwd(None) == E_INVALID and b"lengths_host" in lib.hificar_last_error()
    assert fwd(torch.tensor([T + 1, 3, 1], dtype=torch.int32)) == E_INVALID
    assert fwd(torch.tensor([1, 0, 0], dtype=torch.int32)) == E_INVALID and b"sum of lengths = 1" in lib.hificar_last_error()
    assert fwd(host, ws_bytes=lib.hificar_xfmr_train_workspace_bytes_packed(h, B, mp) - 1) == E_WORKSPACE
    assert fwd(host, tape_bytes=tb - 1) == E_WORKSPACE
    # no packed tape yet: the packed backward has nothing to run on
    assert bwd(host) == E_STATE and b"hificar_xfmr_forward_train_packed" in lib.hificar_last_error()
    # a ragged tape: its backward is the plain one
    assert lib.hificar_xfmr_forward_train_ragged(h, x.data_ptr(), on_dev.data_ptr(), host.data_ptr(), out.data_ptr(), stats.data_ptr(), B, T, p, 1, 0, tape_ptr,
                                                 tb_all, ws_ptr, wb, stream) == 0
    assert bwd(host) == E_STATE
    assert bwd_plain() == 0
    ragged_grads = grads.clone()
    # a packed tape: the plain backward refuses it, other lengths are refused, too small a tape or workspace too; then the right call runs
    assert fwd(host) == 0
    assert bwd_plain() == E_STATE and b"hificar_xfmr_backward_packed" in lib.hificar_last_error()
    other = torch.tensor([lengths[0], lengths[1] - 1, lengths[2] + 1], dtype=torch.int32)  # the same sum, the same Mp
    assert lib.hificar_xfmr_packed_rows(B, T, other.data_ptr()) == mp
    assert bwd(other) == E_INVALID and b"lengths differ" in lib.hificar_last_error()
    assert bwd(host, tape_bytes=tb - 1) == E_WORKSPACE and bwd(host, ws_bytes=lib.hificar_xfmr_train_workspace_bytes_packed(h, B, mp) - 1) == E_WORKSPACE
    assert bwd(host) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(grads).all() and float((grads - ragged_grads).abs().max()) < 1e-2 * float(ragged_grads.abs().max())
    # a dense forward into the same memory makes it a dense tape again
    assert lib.hificar_xfmr_forward_train(h, x.data_ptr(), out.data_ptr(), stats.data_ptr(), B, T, p, 1, 0, tape_ptr, tb_all, ws_ptr, wb, stream) == 0
    assert bwd(host) == E_STATE and bwd_plain() == 0
    torch.cuda.synchronize()
    # the Python surface: a refused call draws no mask and tracks no batch
    before = (m._calls, int(m.conv_blocks[0].bn1.num_batches_tracked))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m.forward_padded(torch.zeros(2, 12, 5, device="cuda:0"), [1, 0], packed=True)
    with pytest.raises(RuntimeError, match=r"lengths must lie in \[0, 5\]"):
        m.forward_padded(torch.zeros(2, 12, 5, device="cuda:0"), [5, 6], packed=True)
    assert (m._calls, int(m.conv_blocks[0].bn1.num_batches_tracked)) == before
