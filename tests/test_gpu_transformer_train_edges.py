"""Transformer training on a MI355X where tests/test_gpu_transformer_train.py does not go: every head size HIFICAR_XFMR_BY_D instantiates that
it leaves out (32, 48, 64, 80, 112), an attention tile whose band no end of the sequence clips, row counts at which the element-wise
grid-stride loops make a second trip and the two-stage sums see many chunks, and channel counts with more than one channel tile
(``transformer_train_oracle.EDGE_SHAPES``; each entry says which kernel form it reaches).  The reference is the float64 restatement
tests/transformer_train_oracle.py taken on the device's ReLU sides, the bars are ``transformer_train_oracle.BARS`` unchanged, and
tests/test_transformer_train_host.py admits every shape on the CPU first.  ``pytest -m gpu``.

rows4112's float64 restatement runs on the GPU (12.6 M feed-forward values: under a second there, several on a host); it is stock PyTorch in
float64 either way, and test_device_reference_of_rows4112_is_the_host_reference holds that run to the host's, once.
"""

import pytest
import torch

import transformer_train_oracle as O
from test_gpu_transformer_train import assert_within, build, dev, reference, step

pytestmark = pytest.mark.gpu

REFERENCE_ON_THE_DEVICE = ("rows4112",)
_RUNS = {}


def run(name):
    """One step of an EDGE_SHAPES entry on the device and its reference, computed once per module and left unchanged: (device results,
    reference, the device's ReLU sides, num_batches_tracked before and after, the model's count of training forwards)."""
    if name not in _RUNS:
        m, x, t = build(name, shapes=O.EDGE_SHAPES)
        before = [int(bn.num_batches_tracked) for bn in m._batch_norms()]  # (the synthetic state_dict's counters are not zero)
        gates = {}
        got = step(m, x, t, gates=gates)
        after = [int(bn.num_batches_tracked) for bn in m._batch_norms()]
        calls = m._calls
        del m
        ref = reference(name, gates, shapes=O.EDGE_SHAPES, device="cuda:0" if name in REFERENCE_ON_THE_DEVICE else "cpu")
        _RUNS[name] = (got, ref, gates, before, after, calls)
    return _RUNS[name]


@pytest.mark.parametrize("name", list(O.EDGE_SHAPES))
def test_edge_step_against_the_restatement(name):
    """Output, loss, batch statistics, running buffers, dx and every gradient (the relative-position tables among them) within BARS of
    the float64 restatement; num_batches_tracked moved by one."""
    got, ref, _, before, after, calls = run(name)
    params, B, T, _ = O.EDGE_SHAPES[name]
    assert got["out"].shape == (B, params["out_channels"], T) and got["out"].dtype == torch.float32
    assert got["dx"].shape == (B, params["in_channels"], T) and torch.isfinite(got["dx"]).all()
    assert set(got["grads"]) == set(ref["grads"])
    assert sum(k.endswith("relative_positional.embeddings") for k in got["grads"]) == params["elayers"]
    errs = O.errors(got, ref)
    assert len(errs) == 4 + len(ref["running"]) + len(ref["grads"])  # out, loss, stats, dx + every running buffer and gradient
    assert_within(errs, name)  # (prints the five largest shares of a bar)
    k = max(errs, key=lambda q: errs[q][0] / errs[q][1])
    print(f"  {name}: worst deviation {k} {errs[k][0]:.3g} (bar {errs[k][1]:g})")
    assert after == [n + 1 for n in before] and calls == 1
    assert "libhificar.so" in open("/proc/self/maps").read()


def test_device_reference_of_rows4112_is_the_host_reference():
    """The float64 restatement of rows4112 as the GPU's library computed it against the same restatement (same gates) on the host, in the
    admission test's terms: within half of every bar (measured: 3.4e-10 of a bar, the output).  The reference does not rest on the device
    library unseen."""
    name = "rows4112"
    assert name in REFERENCE_ON_THE_DEVICE
    _, ref, gates, _, _, _ = run(name)
    assert all(v.device.type == "cuda" for v in ref["grads"].values())
    host = O.restatement(name, torch.float64, gates=gates, shapes=O.EDGE_SHAPES)
    assert all(v.device.type == "cpu" for v in host["grads"].values())
    assert (host["gate_flips"], host["gate_gap"] < O.GATE_GAP) == (ref["gate_flips"], True)
    worst = {k: e / bar for k, (e, bar) in O.errors(ref, host).items()}
    k = max(worst, key=worst.get)
    print(f"  {name}: device float64 against host float64, worst share of a bar: {k} {worst[k]:.3g}")
    assert worst[k] <= 0.5, (k, worst[k])


@pytest.mark.parametrize("name", ["rows1380", "io"])
def test_tape_less_forward_is_bitwise_the_step_with_a_tape(name):
    """Under torch.no_grad() in train() mode (tape = NULL: the rows live in the workspace) the output, the batch statistics and the running
    buffers are bitwise those of the step with a tape, at a row count with a second grid-stride trip and at three output channel tiles."""
    got = run(name)[0]
    m, x, _ = build(name, shapes=O.EDGE_SHAPES)
    with torch.no_grad():
        y = m(dev(x))
    assert not y.requires_grad and m._calls == 1
    assert torch.equal(y, got["out"])
    assert torch.equal(m._last_stats, got["stats"])
    running = {k: v for k, v in m.named_buffers() if k.endswith(("running_mean", "running_var"))}
    assert set(running) == set(got["running"])
    for k, v in running.items():
        assert torch.equal(v, got["running"][k]), k
