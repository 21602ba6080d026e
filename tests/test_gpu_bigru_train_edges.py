"""BiGRU training on a MI355X where the kernels change form and no golden case reaches: a second and third 64-frame head tile, the head at
``kBigruMaxOut`` output channels, every grid-stride loop's second trip, recurrences of the workload's length, the ``<128, 2>`` / ``<192, 2>``
sweeps and other dropout probabilities, against the float64 restatement (shapes and their CPU admission: tests/bigru_train_oracle.py
``EDGE_SHAPES``, tests/test_bigru_train_host.py); and that no result depends on a byte of the tape, the workspace or an output buffer that the
call itself did not write.  The bars are those of tests/test_gpu_bigru_train.py.  ``pytest -m gpu``.
"""

import ctypes

import numpy as np
import pytest
import torch

import bigru_train_oracle as O
from test_gpu_bigru_train import TOL_GRAD, TOL_LOSS, TOL_OUT, build, dev, step
from articulatory_amd import _native
from articulatory_amd.models.bigru import FC1_DIM, _grad_layout
from articulatory_amd.utils.synth import synth_bigru_state_dict, uniform

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(O.EDGE_SHAPES))
def test_edge_shape_against_float64_restatement(name, monkeypatch):
    assert (O.EDGE_BARS["out"], O.EDGE_BARS["loss"], O.EDGE_BARS["grad"]) == (TOL_OUT, TOL_LOSS, TOL_GRAD)
    params, sd, x, t, ns = O.edge_case(name)
    if ns is not None:
        monkeypatch.setenv("HIFICAR_BIGRU_NS", str(ns))
    ref = O.edge_restatement(name, torch.float64)
    assert ref["kink"] > O.KINK_MARGIN  # kink-free
    m = build(params, sd)
    y, loss, grads, dx = step(m, x, t)  # (with the input gradient: bigru_unrows_kernel on every time tile)
    assert y.shape == ref["y"].shape and y.dtype == torch.float32 and dx.shape == ref["dx"].shape
    got = dict(y=y, loss=loss, dx=dx, running_mean=m.bn.running_mean, running_var=m.bn.running_var)
    got.update({"grad." + k: g for k, g in grads.items()})
    errs = O.edge_errors(got, ref, params["dropout"])
    assert sorted(k for k in errs if k.startswith("grad.")) == sorted("grad." + k for k in grads)
    worst = max((k for k in errs if k.startswith("grad.")), key=lambda k: errs[k][0])
    print(f"{name}: y {errs['y'][0]:.3g}, loss {errs['loss'][0]:.3g}, running_mean {errs['running_mean'][0]:.3g}, "
          f"running_var {errs['running_var'][0]:.3g}, dx {errs['dx'][0]:.3g}, worst grad {worst} {errs[worst][0]:.3g}")
    for k, (e, bar) in errs.items():
        assert e < bar, (k, e)
    assert int(m.bn.num_batches_tracked) == int(sd["bn.num_batches_tracked"]) + 1
    assert "libhificar.so" in open("/proc/self/maps").read()


# ------------------------------------------------------------------------------------------------
# scratch: the C entry points on buffers the test owns, once zero-filled and once filled with 0xFF bytes (every float a NaN)
# ------------------------------------------------------------------------------------------------
def owned(nbytes, fill):
    """(the tensor that keeps it alive, a 256-byte aligned device pointer to ``nbytes`` bytes of ``fill``, bytes from there to the end)."""
    buf = torch.full((int(nbytes) + 256,), fill, dtype=torch.uint8, device="cuda:0")
    off = (-buf.data_ptr()) % 256
    return buf, buf.data_ptr() + off, buf.numel() - off


def owned_floats(shape, fill):
    t = torch.full((int(np.prod(shape)) * 4,), fill, dtype=torch.uint8, device="cuda:0").view(torch.float32).view(shape)
    assert t.data_ptr() % 16 == 0
    return t


def native_step(m, x, dout, p, fill, with_tape=True):
    """hificar_bigru_forward_train (+ hificar_bigru_backward with a tape) in the argument order of BiGRU._run_forward_train and
    _BiGRUFunction.backward, every scratch and output buffer pre-filled with ``fill`` bytes: (out, batch statistics, grads, dx)."""
    lib, h = m._lib, m._handle
    B, C, T = x.shape
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = owned_floats((B, m._params["out_channels"], T), fill)
    stats = owned_floats((2, FC1_DIM), fill)
    ws, ws_ptr, ws_bytes = owned(lib.hificar_bigru_train_workspace_bytes(h, B, T), fill)
    tape, tape_ptr, tape_bytes = owned(lib.hificar_bigru_tape_bytes(h, B, T), fill) if with_tape else (None, None, 0)
    _native.check(lib.hificar_bigru_forward_train(h, x.data_ptr(), out.data_ptr(), stats.data_ptr(), B, T, float(p), 4242, 3, tape_ptr, tape_bytes,
                                                  ws_ptr, ws_bytes, stream), "hificar_bigru_forward_train")
    if not with_tape:
        torch.cuda.synchronize()
        return out, stats, None, None
    grads = owned_floats((int(lib.hificar_bigru_grad_floats(h)),), fill)
    dx = owned_floats((B, C, T), fill)
    _native.check(lib.hificar_bigru_backward(h, dout.data_ptr(), B, T, tape_ptr, tape_bytes, grads.data_ptr(), dx.data_ptr(), ws_ptr, ws_bytes, stream),
                  "hificar_bigru_backward")
    torch.cuda.synchronize()
    return out, stats, grads, dx


# (Cin, H, out, B, T, p, tanh): B T = 15 far inside the slack rows and the batch norm's 32 row lanes | Cin padded to 32, two head tiles, tanh' | H 256
SCRATCH_SHAPES = {
    "b3_t5": (8, 64, 12, 3, 5, 0.3, False),
    "cin13_t70_tanh": (13, 64, 12, 2, 70, 0.3, True),
    "h256": (24, 256, 18, 2, 16, 0.3, False),
}


@pytest.mark.parametrize("name", list(SCRATCH_SHAPES))
def test_results_do_not_depend_on_scratch_the_call_did_not_write(name):
    """Zero-filled against NaN-filled tape, workspace, out, batch statistics, gradient buffer and dx: bitwise the same results (every
    reduction runs in a fixed order), in every gradient slot of hificar_bigru_grad_info (the padding floats between slots are not promised)."""
    cin, H, out_ch, B, T, p, tanh = SCRATCH_SHAPES[name]
    params = dict(in_channels=cin, hidden_size=H, out_channels=out_ch, use_tanh=tanh, dropout=p)
    seed = 7200 + list(SCRATCH_SHAPES).index(name)
    m = build(params, synth_bigru_state_dict(params, seed=seed))
    m._native_handle(train=True)
    x = dev(uniform(seed, "x", (B, cin, T), -1.0, 1.0))
    dout = dev(uniform(seed, "dout", (B, out_ch, T), -1.0, 1.0))
    layout = _grad_layout(m)
    assert sorted(n for n, _, _ in layout) == sorted(n for n, _ in m.named_parameters())
    clean = native_step(m, x, dout, p, 0x00)
    dirty = native_step(m, x, dout, p, 0xFF)
    assert torch.isnan(owned_floats((4,), 0xFF)).all()  # the poison is what it claims to be
    for what, a, b in zip(("out", "batch statistics"), clean[:2], dirty[:2]):
        assert torch.isfinite(b).all(), what
        assert torch.equal(a, b), what
    assert torch.isfinite(dirty[3]).all() and torch.equal(clean[3], dirty[3]), "dx"
    for key, off, num in layout:
        assert torch.isfinite(dirty[2][off:off + num]).all(), key
        assert torch.equal(clean[2][off:off + num], dirty[2][off:off + num]), key
    assert float(clean[3].abs().max()) > 0 and all(float(clean[2][off:off + num].abs().max()) > 0 for _, off, num in layout)  # (something was computed)
    # tape = NULL, the forward-only path: its rows live in the workspace
    light_clean = native_step(m, x, dout, p, 0x00, with_tape=False)
    light_dirty = native_step(m, x, dout, p, 0xFF, with_tape=False)
    assert torch.isfinite(light_dirty[0]).all() and torch.equal(light_clean[0], light_dirty[0])
    assert torch.equal(light_clean[1], light_dirty[1])
    assert torch.equal(light_clean[0], clean[0])  # the same arithmetic with and without a tape


def test_a_small_step_after_a_large_one_on_the_grown_workspace():
    """The training analogue of tests/test_gpu_bigru.py::test_repeatable_and_workspace_regrows: a (B 2, T 9) step on a workspace that a
    (B 6, T 130) step has used is bitwise the step of a model that never saw the large shape."""
    params, _, _, seed = O.case_params("c0")
    sd = O.case_state_dict("c0")
    cin, out_ch = params["in_channels"], params["out_channels"]

    def batch(tag, B, T):
        x = uniform(seed, "regrow.x." + tag, (B, cin, T), -1.0, 1.0)
        t = uniform(seed, "regrow.t." + tag, (B, out_ch, T), 4.0, 5.0)
        return x, t

    a = build(params, sd, seed=991)
    step(a, *batch("large", 6, 130))
    large_ws = a._train_ws_buf.numel()
    ya, _, ga, dxa = step(a, *batch("small", 2, 9))
    assert a._train_ws_buf.numel() == large_ws  # grow-only: the small step ran in the large step's buffer
    b = build(params, sd, seed=991)
    b.set_dropout_seed(991, offset=1)
    yb, _, gb, dxb = step(b, *batch("small", 2, 9))
    assert b._train_ws_buf.numel() < large_ws
    assert torch.equal(ya, yb) and torch.equal(dxa, dxb)
    assert sorted(ga) == sorted(gb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
