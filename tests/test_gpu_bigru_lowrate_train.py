"""BiGRU training on low-rate inputs on a MI355X: ``BiGRU.forward_lowrate_train`` through ``hificar_bigru_forward_train_lowrate`` /
``hificar_bigru_backward_lowrate`` against the float64 restatement tests/bigru_lowrate_train_oracle.py (shapes and their CPU admission:
``LOW_SHAPES``, tests/test_bigru_lowrate_train_host.py), against the device's own step on the materialised stretch, bitwise against the existing
entry points at factor 1, bitwise independence of padded frames and scratch, and the trainer's ``lowrate_interp_factor``.  The bars are those of
tests/test_gpu_bigru_train.py.  ``pytest -m gpu``.

Run as a script with shape names (``python tests/test_gpu_bigru_lowrate_train.py e e_p0``) it checks those shapes against the restatement in
this process: how case E gets its ``HIFICAR_BIGRU_NS=2`` in a fresh process.
"""

import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO  # (first: it puts the repository on sys.path, also when this file runs as a script)

import bigru_lowrate_train_oracle as L
import bigru_train_oracle as O
from test_gpu_bigru_train import TOL_GRAD, TOL_LOSS, TOL_OUT, build, dev, steps_config
from test_gpu_bigru_train_edges import owned, owned_floats
from articulatory_amd import _native
from articulatory_amd.bin import train as T
from articulatory_amd.losses import masked_l1_loss
from articulatory_amd.models import BiGRU
from articulatory_amd.models.bigru import FC1_DIM, _grad_layout
from articulatory_amd.utils.synth import uniform

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(name):
    return L.low_restatement(name, torch.float64)  # computed once per shape, never modified


def low_pad(lengths, Tl):
    """(B, Tl) bool: the padded low-rate frames."""
    return (torch.arange(Tl)[None, :] >= torch.as_tensor(list(lengths))[:, None]).to("cuda:0")


def lstep(m, x, t, f, lengths, zs, need_dx=True):
    """One forward_lowrate_train + backward of the (masked) L1 loss on the device: dict(y, loss, dx, running_*, grad.<key>)."""
    for p in m.parameters():
        p.grad = None
    xt = dev(x).requires_grad_(need_dx and not zs)
    y = m.forward_lowrate_train(xt, lengths, interp_factor=f, zscore=zs)
    loss = F.l1_loss(y, dev(t)) if lengths is None else masked_l1_loss(y, dev(t), f * torch.as_tensor(list(lengths), dtype=torch.int32))
    loss.backward()
    got = dict(y=y.detach(), loss=loss.detach(), dx=xt.grad, running_mean=m.bn.running_mean.clone(), running_var=m.bn.running_var.clone())
    got.update({"grad." + k: p.grad.detach().clone() for k, p in m.named_parameters()})
    return got


def mstep(m, x, t, f, lengths):
    """The same step on the MATERIALISED stretch: stock F.interpolate on the device (every sequence by its own length), then forward /
    forward_padded; dx pulled back through torch's interpolate."""
    for p in m.parameters():
        p.grad = None
    xl = dev(x).requires_grad_(True)
    if lengths is None:
        y = m(F.interpolate(xl, size=f * x.shape[2], mode="linear", align_corners=False))
        loss = F.l1_loss(y, dev(t))
    else:
        Tl = x.shape[2]
        rows = [torch.cat([F.interpolate(xl[b:b + 1, :, :l], size=f * l, mode="linear", align_corners=False)[0] if l else xl.new_zeros((x.shape[1], 0)),
                           xl.new_zeros((x.shape[1], f * (Tl - l)))], dim=1) for b, l in enumerate(lengths)]
        hi = f * torch.as_tensor(list(lengths), dtype=torch.int32)
        y = m.forward_padded(torch.stack(rows), hi)
        loss = masked_l1_loss(y, dev(t), hi)
    loss.backward()
    got = dict(y=y.detach(), loss=loss.detach(), dx=xl.grad, running_mean=m.bn.running_mean.clone(), running_var=m.bn.running_var.clone())
    got.update({"grad." + k: p.grad.detach().clone() for k, p in m.named_parameters()})
    return got


def check_case(name):
    """A LOW_SHAPES entry on the device against the float64 restatement, every figure printed before it is held to its bar."""
    assert (O.EDGE_BARS["out"], O.EDGE_BARS["loss"], O.EDGE_BARS["grad"]) == (TOL_OUT, TOL_LOSS, TOL_GRAD)
    params, sd, x, t, f, lengths, ns, zs = L.low_case(name)
    assert ns is None or os.environ.get("HIFICAR_BIGRU_NS") == str(ns)
    ref = reference(name)
    assert ref["kink"] > O.KINK_MARGIN
    m = build(params, sd)
    got = lstep(m, x, t, f, lengths, zs)
    assert got["y"].shape == ref["y"].shape == (x.shape[0], params["out_channels"], f * x.shape[2]) and got["y"].dtype == torch.float32
    assert zs or got["dx"].shape == tuple(x.shape)
    errs = O.edge_errors(got, ref, params["dropout"])
    assert ("dx" in errs) == (not zs) and sum(k.startswith("grad.") for k in errs) == 22
    worst = max((k for k in errs if k.startswith("grad.")), key=lambda k: errs[k][0])
    print(f"{name}: y {errs['y'][0]:.3g}, loss {errs['loss'][0]:.3g}, running_mean {errs['running_mean'][0]:.3g}, running_var "
          f"{errs['running_var'][0]:.3g}, dx {errs['dx'][0] if 'dx' in errs else float('nan'):.3g}, worst grad {worst} {errs[worst][0]:.3g}")
    for k, (e, bar) in errs.items():
        assert e < bar, (k, e)
    if lengths is not None:
        pad = low_pad(lengths, x.shape[2])
        assert float(got["dx"].transpose(1, 2)[pad].abs().max()) == 0.0                                   # exactly zero
        assert float(got["y"].transpose(1, 2)[pad.repeat_interleave(f, dim=1)].abs().max()) == 0.0
    assert all(torch.isfinite(v).all() for v in got.values() if v is not None)
    assert int(m.bn.num_batches_tracked) == int(sd["bn.num_batches_tracked"]) + 1 and m._calls == 1
    assert "libhificar.so" in open("/proc/self/maps").read()


# ------------------------------------------------------------------------------------------------ 1: cases A - D and zscore
@pytest.mark.parametrize("name", [n for n, s in L.LOW_SHAPES.items() if s[9] is None])
def test_low_rate_shape_against_float64_restatement(name):
    check_case(name)


@pytest.mark.parametrize("name", L.GOLD)
def test_golden_case_of_the_reference(name):
    """The reference's own BiGRU in train() mode on F.interpolate'd input (tools/make_golden_bigru_lowrate_train.py), same bars."""
    gold = np.load(os.path.join(REPO, "tests", "golden", "gold_bigru_lowrate_train.npz"))
    params, sd, x, t, f, lengths, _, zs = L.low_case(name)
    got = lstep(build(params, sd), x, t, f, lengths, zs)
    devs = {k: O.deviation(gold, f"{name}_{k}", v) for k, v in got.items() if k != "loss"}
    loss_err = abs(float(got["loss"]) - float(gold[name + "_loss"])) / abs(float(gold[name + "_loss"]))
    print(f"{name}: y {devs['y']:.3g}, loss {loss_err:.3g}, dx {devs['dx']:.3g}, worst grad {max(v for k, v in devs.items() if k.startswith('grad.')):.3g}")
    assert len(devs) == 26 and loss_err < TOL_LOSS
    for k, e in devs.items():
        assert e < (TOL_OUT if k in ("y", "running_mean", "running_var") else TOL_GRAD), (k, e)


def test_case_e_two_sequences_per_workgroup_in_a_fresh_process():
    """Case D with HIFICAR_BIGRU_NS=2 (the A/B switch of the sweeps' tile height), so that an unequal pair shares a sweep tile."""
    names = [n for n, s in L.LOW_SHAPES.items() if s[9] == 2]
    assert names == ["e", "e_p0"]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *names], env=dict(os.environ, HIFICAR_BIGRU_NS="2"), cwd=REPO, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and all(f"{n}: y " in r.stdout for n in names)


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("name", ["a17", "b_f3", "c", "d", "d_p0"])
def test_against_the_devices_own_materialised_step(name):
    """forward / forward_padded on stock F.interpolate's stretch, same seed and offset: both runs lie within one bar of the same float64
    values, so they agree within twice the bar (not bitwise: the projection is commuted)."""
    params, sd, x, t, f, lengths, _, zs = L.low_case(name)
    low = lstep(build(params, sd), x, t, f, lengths, zs)
    mat = {k: v.double().cpu() for k, v in mstep(build(params, sd), x, t, f, lengths).items()}
    errs = O.edge_errors(low, mat, params["dropout"])
    worst = max(errs, key=lambda k: errs[k][0] / errs[k][1])
    print(f"{name}: y {errs['y'][0]:.3g}, dx {errs['dx'][0]:.3g}, worst share of twice the bar {worst} {errs[worst][0] / (2 * errs[worst][1]):.3g}")
    assert "dx" in errs and sum(k.startswith("grad.") for k in errs) == 22
    for k, (e, bar) in errs.items():
        assert e < 2 * bar, (k, e)


# ------------------------------------------------------------------------------------------------ the C entry points on owned buffers
def native_low(m, x, dout, p, fill, f, zs=0, lengths=None, with_tape=True, need_dx=True, existing=False):
    """hificar_bigru_forward_train_lowrate then hificar_bigru_backward_lowrate (existing: hificar_bigru_forward_train[_ragged] and
    hificar_bigru_backward, on the same input) with every scratch and output buffer pre-filled with ``fill`` bytes: (out, batch statistics,
    grads, dx, tape bytes as a tensor)."""
    lib, h = m._lib, m._handle
    B, C, Tl = x.shape
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = owned_floats((B, m._params["out_channels"], f * Tl), fill)
    stats = owned_floats((2, FC1_DIM), fill)
    if existing:
        wsn, tpn = lib.hificar_bigru_train_workspace_bytes(h, B, Tl), lib.hificar_bigru_tape_bytes(h, B, Tl)
    else:
        wsn, tpn = lib.hificar_bigru_train_workspace_bytes_lowrate(h, B, Tl, f), lib.hificar_bigru_tape_bytes_lowrate(h, B, Tl, f)
    assert wsn > 0 and tpn > 0
    ws, ws_ptr, ws_bytes = owned(wsn, fill)
    tape, tape_ptr, tape_bytes = owned(tpn, fill) if with_tape else (None, None, 0)
    host = on_dev = None
    if lengths is not None:
        host = torch.tensor(list(lengths), dtype=torch.int32)
        on_dev = host.to("cuda:0")
    lp = (on_dev.data_ptr(), host.data_ptr()) if lengths is not None else (None, None)
    tail = (float(p), 4242, 3, tape_ptr, tape_bytes, ws_ptr, ws_bytes, stream)
    if not existing:
        rc = lib.hificar_bigru_forward_train_lowrate(h, x.data_ptr(), *lp, out.data_ptr(), stats.data_ptr(), B, Tl, f, zs, *tail)
    elif lengths is None:
        rc = lib.hificar_bigru_forward_train(h, x.data_ptr(), out.data_ptr(), stats.data_ptr(), B, Tl, *tail)
    else:
        rc = lib.hificar_bigru_forward_train_ragged(h, x.data_ptr(), *lp, out.data_ptr(), stats.data_ptr(), B, Tl, *tail)
    _native.check(rc, "forward")
    if not with_tape:
        torch.cuda.synchronize()
        return out, stats, None, None, None
    grads = owned_floats((int(lib.hificar_bigru_grad_floats(h)),), fill)
    dx = owned_floats((B, C, Tl), fill) if need_dx else None
    dxp = dx.data_ptr() if need_dx else None
    if existing:
        rc = lib.hificar_bigru_backward(h, dout.data_ptr(), B, Tl, tape_ptr, tape_bytes, grads.data_ptr(), dxp, ws_ptr, ws_bytes, stream)
    else:
        rc = lib.hificar_bigru_backward_lowrate(h, dout.data_ptr(), B, Tl, f, zs, tape_ptr, tape_bytes, grads.data_ptr(), dxp, ws_ptr, ws_bytes, stream)
    _native.check(rc, "backward")
    torch.cuda.synchronize()
    off = (-tape.data_ptr()) % 256
    return out, stats, grads, dx, tape[off:off + tpn]


def native_model(name, B=None, Tl=None):
    params, sd, x, t, f, lengths, _, zs = L.low_case(name)
    seed = L.LOW_SEEDS[name]
    B, Tl = B or x.shape[0], Tl or x.shape[2]
    m = build(params, sd)
    m._native_handle(train=True)
    x = dev(uniform(seed, "x", (B, params["in_channels"], Tl), -1.0, 1.0))
    dout = dev(uniform(seed, "dout", (B, params["out_channels"], f * Tl), -1.0, 1.0))
    return m, params, x, dout, f, lengths


def same(a, b, m, what=""):
    assert torch.equal(a[0], b[0]), what + " out"
    assert torch.equal(a[1], b[1]), what + " batch statistics"
    if a[2] is None:
        return
    assert (a[3] is None and b[3] is None) or torch.equal(a[3], b[3]), what + " dx"
    for key, off, num in _grad_layout(m):
        assert torch.isfinite(b[2][off:off + num]).all(), key
        assert torch.equal(a[2][off:off + num], b[2][off:off + num]), what + " " + key


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", ["a17", "d"])
def test_factor_one_is_bitwise_the_existing_entry_points(name):
    m, params, x, dout, _, lengths = native_model(name)
    B, _, Tl = x.shape
    dout = dout[:, :, :Tl].contiguous()
    lib, h = m._lib, m._handle
    assert lib.hificar_bigru_tape_bytes_lowrate(h, B, Tl, 1) == lib.hificar_bigru_tape_bytes(h, B, Tl)
    assert lib.hificar_bigru_train_workspace_bytes_lowrate(h, B, Tl, 1) == lib.hificar_bigru_train_workspace_bytes(h, B, Tl)
    p = params["dropout"]
    old = native_low(m, x, dout, p, 0x00, 1, lengths=lengths, existing=True)
    new = native_low(m, x, dout, p, 0x00, 1, lengths=lengths)
    same(old, new, m)
    assert torch.equal(old[4], new[4])  # the same launches: the same tape, byte for byte
    assert float(new[3].abs().max()) > 0
    # through the module: forward_lowrate_train(interp_factor=1) is forward / forward_padded
    _, sd, xs, t, _, _, _, _ = L.low_case(name)
    t = t[:, :, :Tl]
    a, b = build(params, sd), build(params, sd)
    ga = lstep(a, xs, t, 1, lengths, False)
    for q in b.parameters():
        q.grad = None
    xt = dev(xs).requires_grad_(True)
    yb = b(xt) if lengths is None else b.forward_padded(xt, lengths)
    (F.l1_loss(yb, dev(t)) if lengths is None else masked_l1_loss(yb, dev(t), torch.as_tensor(list(lengths), dtype=torch.int32))).backward()
    assert torch.equal(ga["y"], yb.detach()) and torch.equal(ga["dx"], xt.grad) and torch.equal(ga["running_var"], b.bn.running_var)
    for k, q in b.named_parameters():
        assert torch.equal(ga["grad." + k], q.grad), k


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("name,B,Tl", [("a17", 3, 17), ("d", 2, 24), ("z", 2, 43)])
def test_all_lengths_full_is_bitwise_the_dense_low_rate_call(name, B, Tl):
    m, params, x, dout, f, _ = native_model(name, B, Tl)
    zs = 1 if L.LOW_SHAPES[name][10] else 0
    p = params["dropout"]
    dense = native_low(m, x, dout, p, 0x00, f, zs, need_dx=not zs)
    ragged = native_low(m, x, dout, p, 0x00, f, zs, lengths=[Tl] * B, need_dx=not zs)
    same(dense, ragged, m)
    assert all(float(dense[2][off:off + num].abs().max()) > 0 for _, off, num in _grad_layout(m))
    light = native_low(m, x, dout, p, 0x00, f, zs, lengths=[Tl] * B, with_tape=False)
    assert torch.equal(light[0], dense[0]) and torch.equal(light[1], dense[1])


# ------------------------------------------------------------------------------------------------ 5
def test_results_depend_neither_on_padded_frames_nor_on_scratch(monkeypatch):
    """x and dout zero in the padded frames on zero-filled buffers, against NaN there on 0xFF-filled buffers (tape, workspace, out, statistics,
    gradient buffer, dx): finite and bitwise equal, with and without a tape, at one and at two sequences per workgroup."""
    for ns in ("1", "2"):
        monkeypatch.setenv("HIFICAR_BIGRU_NS", ns)
        m, params, x, dout, f, lengths = native_model("d")
        pad = low_pad(lengths, x.shape[2])[:, None, :]
        pad_h = pad.repeat_interleave(f, dim=2)
        assert bool(pad.any())
        p = params["dropout"]
        xz, dz = x.masked_fill(pad, 0.0).contiguous(), dout.masked_fill(pad_h, 0.0).contiguous()
        xn, dn = x.masked_fill(pad, float("nan")).contiguous(), dout.masked_fill(pad_h, float("nan")).contiguous()
        clean = native_low(m, xz, dz, p, 0x00, f, lengths=lengths)
        dirty = native_low(m, xn, dn, p, 0xFF, f, lengths=lengths)
        assert torch.isnan(owned_floats((4,), 0xFF)).all()
        assert torch.isfinite(dirty[0]).all() and torch.isfinite(dirty[1]).all() and torch.isfinite(dirty[3]).all()
        same(clean, dirty, m, "ns " + ns)
        assert float(dirty[3].transpose(1, 2)[pad[:, 0, :]].abs().max()) == 0.0 and float(dirty[0].transpose(1, 2)[pad_h[:, 0, :]].abs().max()) == 0.0
        assert float(clean[3].abs().max()) > 0 and all(float(clean[2][off:off + num].abs().max()) > 0 for _, off, num in _grad_layout(m))
        light_clean = native_low(m, xz, dz, p, 0x00, f, lengths=lengths, with_tape=False)
        light_dirty = native_low(m, xn, dn, p, 0xFF, f, lengths=lengths, with_tape=False)
        assert torch.isfinite(light_dirty[0]).all() and torch.isfinite(light_dirty[1]).all()
        same(light_clean, light_dirty, m, "tape-less")
        same(light_clean, clean[:2] + (None, None), m, "with and without a tape")
        # the tape's low-rate input rows, dW_ih's operand, are zeros on padded frames whatever x holds there
        cp = 32  # in_channels 24 rounded up to 32; the rows lie behind the tape's 256-byte header
        rows = dirty[4][256:256 + x.shape[0] * x.shape[2] * cp * 4].view(torch.float32).view(x.shape[0], x.shape[2], cp)
        assert float(rows[pad[:, 0, :]].abs().max()) == 0.0 and torch.isfinite(rows).all()
        assert torch.equal(rows[:, :, :24], xz.transpose(1, 2)) and float(rows[:, :, 24:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 6
def test_a_sequence_does_not_depend_on_its_neighbours():
    """Sequence 0 alone and inside case D at p = 0.  In train() mode the batch norm ties every output to the whole batch, so what can be
    equal bit for bit is what lies in front of it: the tape's low-rate rows and layer 1's hidden states (the low-rate projection, the
    interpolated pre-gates and the sweep), read from the tapes; and, in eval mode, the output itself."""
    m, params, x, dout, f, lengths = native_model("d_p0")
    B, C, Tl = x.shape
    H, cp, Th = params["hidden_size"], 32, f * Tl
    alone = native_low(m, x[:1].contiguous(), dout[:1].contiguous(), 0.0, 0x00, f, lengths=lengths[:1], need_dx=False)
    batch = native_low(m, x, dout, 0.0, 0x00, f, lengths=lengths, need_dx=False)

    def blocks(tape, nb):  # header | [rows of nb Tl + slack][cp] | [rows of nb Th + slack][2H]
        rl, rh = -(-(nb * Tl + 64) // 256) * 256, -(-(nb * Th + 64) // 256) * 256
        x0 = tape[256:256 + Tl * cp * 4].view(torch.float32)
        y1 = tape[256 + rl * cp * 4:256 + rl * cp * 4 + Th * 2 * H * 4].view(torch.float32)
        return x0, y1

    for a, b in zip(blocks(alone[4], 1), blocks(batch[4], B)):
        assert float(a.abs().max()) > 0 and torch.equal(a, b)
    m.eval()
    with torch.no_grad():
        ya = m.forward_lowrate_train(x[:1].contiguous(), lengths[:1], interp_factor=f)
        yb = m.forward_lowrate_train(x, lengths, interp_factor=f)
        assert torch.equal(ya[0], yb[0]) and torch.equal(yb, m.forward_lowrate(x, lengths, interp_factor=f))  # eval(): forward_lowrate


# ------------------------------------------------------------------------------------------------ 7
def test_repeatable_and_the_tape_less_form_without_grad():
    params, sd, x, t, f, lengths, _, _ = L.low_case("d")
    runs = [lstep(build(params, sd, seed=4242), x, t, f, lengths, False) for _ in range(2)]
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    m = build(params, sd, seed=4242)
    with torch.no_grad():
        y = m.forward_lowrate_train(dev(x), lengths, interp_factor=f)
    assert torch.equal(y, runs[0]["y"]) and torch.equal(m.bn.running_var, runs[0]["running_var"]) and m._calls == 1
    assert not y.requires_grad
    y2 = m.forward_lowrate_train(dev(x), lengths, interp_factor=f)  # the next call draws the next masks
    assert y2.requires_grad and not torch.equal(y2.detach(), y) and m._calls == 2 and int(m.bn.num_batches_tracked) == int(sd["bn.num_batches_tracked"]) + 2
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        m.forward_lowrate_train(dev(x)[:1, :, :1], [0], interp_factor=f)
    assert m._calls == 2


# ------------------------------------------------------------------------------------------------ 8
def test_zscore_is_the_step_on_the_pre_normalised_input():
    params, sd, x, t, f, lengths, _, zs = L.low_case("z")
    assert zs and lengths is None
    got = lstep(build(params, sd), x, t, f, None, True)
    xn = np.stack([((u.astype(np.float64) - u.astype(np.float64).mean()) / u.astype(np.float64).std()) for u in x]).astype(np.float32)
    pre = {k: (v.double().cpu() if v is not None else None) for k, v in lstep(build(params, sd), xn, t, f, None, False, need_dx=False).items()}
    errs = O.edge_errors(got, pre, params["dropout"])
    print("zscore against the pre-normalised input:", {k: f"{e:.3g}" for k, (e, _) in errs.items() if not k.startswith("grad.")},
          "worst grad", max(e for k, (e, _) in errs.items() if k.startswith("grad.")))
    for k, (e, bar) in errs.items():
        assert e < bar, (k, e)
    m = build(params, sd)
    with pytest.raises(NotImplementedError, match="gradient of the input is not built"):
        m.forward_lowrate_train(dev(x).requires_grad_(True), None, interp_factor=f, zscore=True)
    h = m._native_handle(train=True)
    lib, fake = m._lib, 1 << 20
    assert lib.hificar_bigru_backward_lowrate(h, fake, 2, 43, f, 1, fake, 1 << 40, fake, fake, fake, 1 << 40, None) == -1  # dx on a zscore tape


# ------------------------------------------------------------------------------------------------ 9
@pytest.mark.parametrize("mode", ["random_window", "pad"])
def test_five_steps_through_the_trainer(mode, tmp_path):
    N = 4
    gp = dict(in_channels=24, hidden_size=64, out_channels=12, dropout=0.0)
    cfg = dict(steps_config(gp), package_mode=mode, lowrate_interp_factor=N, generator_optimizer_params=dict(lr=1e-2), train_max_steps=5,
               discriminator_train_start_steps=5)
    torch.manual_seed(0)
    tr = T.InversionTrainer(cfg, torch.device("cuda:0"))
    data = T.WindowPairs(synthetic=4, frames=64, dims=(24, 12), seed=0, frames_range=(40, 64) if mode == "pad" else None, x_factor=N)
    collate = T.LowRateWindowCollater(24, 2, N, seed=1) if mode == "random_window" else T.LowRatePadCollater(N, pad_max_frames=48, seed=1)
    batch = collate(data.items)
    assert batch["y"].shape[2] == N * batch["x"].shape[2] and (mode == "pad") == ("lengths" in batch)
    losses = [float(tr.train_step(batch)["train/generator_loss"]) for _ in range(5)]
    print(mode, "losses", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] and tr.steps == 5 and tr.G._calls == 5
    calls = []
    inner = tr.G.forward_lowrate
    tr.G.forward_lowrate = lambda x, **kw: (calls.append(kw), inner(x, **kw))[1]
    dev_batch = T.LowRatePadCollater(N)(data.items)
    tr.G.eval()
    ev = tr.eval_step(dev_batch)
    with torch.no_grad():
        want = masked_l1_loss(inner(dev_batch["x"].to("cuda:0"), lengths=dev_batch["lengths"], interp_factor=N), dev_batch["y"].to("cuda:0"),
                              N * dev_batch["lengths"])
    tr.G.train()
    assert len(calls) == 1 and calls[0]["interp_factor"] == N and calls[0]["zscore"] is False and torch.equal(calls[0]["lengths"], dev_batch["lengths"])
    assert np.isfinite(float(ev["eval/mel_loss"])) and float(ev["eval/mel_loss"]) == float(want)
    del tr.G.forward_lowrate
    tr.save_checkpoint(str(tmp_path / "ckpt.pkl"))
    state = torch.load(tmp_path / "ckpt.pkl", map_location="cpu")
    assert state["steps"] == 5 and sorted(state) == ["dropout", "epochs", "model", "optimizer", "scheduler", "steps"]
    BiGRU(**gp).load_state_dict(state["model"]["generator"], strict=True)  # the reference's layout: nothing about the low rate in a checkpoint


if __name__ == "__main__":
    assert torch.cuda.is_available()
    for case in sys.argv[1:]:
        check_case(case)
