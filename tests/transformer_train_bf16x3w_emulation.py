"""CPU emulation of the Transformer's bf16x3w TRAINING arithmetic (``train_precision="bf16x3w"``), to set the device's accuracy bars before a
GPU sees it ("bf16x3w").

The bf16x3 emulation (tests/transformer_train_bf16x3_emulation.py: its code, imported) with one more reroute: the weight gradient of every
layer the device's GEMM-form rule selects (``gemm_form``: one tap, more than 96 output channels and more than 96 input columns, i.e. at
least four 32-blocks each way — ``w_raw_in``, q | k | v, ``w_o``, ``linear1``, ``linear2``; a one-tap ``residual_path`` only with that many
input channels) is

    dW = G^T A ~ hi(G)^T hi(A) + hi(G)^T lo(A) + lo(G)^T hi(A)        hi(a) = bf16(fp32(a)),  lo(a) = bf16(fp32(a) - hi(a))

and the bias gradient of such a layer is the sum over the rows of hi(G) + lo(G) — what wgrad_bf16x3_kernel builds: its bias sums come from the
split G tile it has staged, not from a separate exact pass.  Every other weight and bias gradient stays exact, as on the device (the k = 3
ResBlock convs, ``w_out``, ``residual_path`` at 12 channels).  Products and sums in float64 (the device: fp32 accumulation, another order;
what the factor 4 is for).

The bars follow the project's rule, per class: E = the largest emulated error over the GPU cases (CASES, EDGE_CASES, RAGGED_CASE, the
five-step run) against the float64 restatement on the emulation's ReLU sides; the device bar is the fp32 bar where E is at most a quarter
of it, otherwise 4 E; the output keeps 2e-4.  EMULATED and BARS_X3W below were recorded from ``python
tests/transformer_train_bf16x3w_emulation.py`` BEFORE the first GPU run of the arithmetic; tests/test_transformer_train_bf16x3w_host.py
recomputes the errors and holds them to a quarter of the bars.  The emulation predicts; the device is never compared against it.  Test
infrastructure only.
"""

import contextlib

import torch
import torch.nn.functional as F

import transformer_ragged_oracle as R
import transformer_train_bf16x3_emulation as E
import transformer_train_oracle as O
from transformer_bf16x3_emulation import split

CASES = ("t2", "t65", "nores")        # of transformer_train_oracle.SHAPES: what tests/test_gpu_transformer_train_bf16x3w.py runs
EDGE_CASES = ("d48", "rows4112", "rows1380")  # ... and of its EDGE_SHAPES
RAGGED_CASE = E.RAGGED_CASE           # transformer_ragged_oracle.RAGGED_SHAPES "mixed": B = 3, T = 70, lengths (70, 33, 1); padded and packed


def gemm_form(cout, cin, K):
    """wgrad_gemm_form (hificar_train.hip.inc) of a (cout, cin, K) weight: one tap, at least four 32-blocks of output channels and of input
    columns (the input rows are padded to a multiple of 32 columns)."""
    return K == 1 and (cout + 31) // 32 >= 4 and (cin + 31) // 32 >= 4


class _Linear3W(torch.autograd.Function):
    """_Linear3 with the bias inside and the weight and bias gradients in bf16x3 (a layer gemm_form selects)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        y = E.mm3(x, w.t())
        return y if b is None else y + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        g, a = dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1])
        gh, gl = split(g)
        return E.mm3(dy, w), E.mm3(g.t(), a), (gh + gl).sum(0) if ctx.has_bias else None


_linear3 = E.linear3  # (emulating() points E.linear3 here)


def linear3w(x, w, b=None):
    return _Linear3W.apply(x, w, b) if gemm_form(w.shape[0], w.shape[1], 1) else _linear3(x, w, b)


def conv3w(x, w, b=None, padding=0):
    if not gemm_form(*w.shape):
        return E.conv3(x, w, b, padding)
    return _Linear3W.apply(x.transpose(1, 2), w[:, :, 0], b).transpose(1, 2)  # (one tap: no padding)


class _FW(E._F):
    linear, conv1d = staticmethod(linear3w), staticmethod(conv3w)


@contextlib.contextmanager
def emulating():
    """E.emulating() with the GEMM-form layers' weight and bias gradients in bf16x3 too (the projection einsums go through E.linear3, looked
    up when they run)."""
    real = torch.einsum
    O.F = R.F = _FW()
    E.linear3 = linear3w
    torch.einsum = E._einsum3(real)
    try:
        yield
    finally:
        O.F = R.F = F
        E.linear3 = _linear3
        torch.einsum = real


def emulated_case(name):
    shapes = O.EDGE_SHAPES if name in O.EDGE_SHAPES else None
    with emulating():
        emu = O.restatement(name, torch.float64, shapes=shapes)
    return emu, O.restatement(name, torch.float64, gates=emu["sides"], shapes=shapes)


def emulated_ragged():
    real = E.emulating
    E.emulating = emulating  # (E.emulated_ragged's own code, under this module's reroute)
    try:
        return E.emulated_ragged()
    finally:
        E.emulating = real


def emulated_errors(verbose=False, cases=CASES + EDGE_CASES):
    """E.emulated_errors over this arithmetic's cases: {class: largest emulated error}, and the largest gate gap."""
    worst, gap = {}, 0.0
    runs = [(name, emulated_case) for name in cases] + [(RAGGED_CASE + " (ragged)", lambda _: emulated_ragged())]
    for name, fn in runs:
        emu, ref = fn(name)
        c = E.classes(O.errors(emu, ref))
        gap = max(gap, ref["gate_gap"])
        if verbose:
            print(f"{name}: {ref['gate_flips']} flips, gap {ref['gate_gap']:.3g}; " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(c.items())))
        for k, v in c.items():
            worst[k] = max(worst.get(k, 0.0), v)
    with emulating():
        losses, final = O.five_steps(torch.float64)
    e_loss, per = O.five_step_errors(losses, final, *O.five_steps(torch.float64))
    worst["steps_loss"], worst["steps_params"] = e_loss, max(per.values())
    if verbose:
        print(f"five steps: loss {e_loss:.3g}, parameters {max(per.values()):.3g} ({max(per, key=per.get)})")
    return worst, gap


# ---- recorded before the first GPU run (see the module's docstring); E: emulated (rounded up in its third digit), bar: what the device is held to
# (The worst cases: out t65; loss, stats, running, dx and grad t2 — at 4 rows its worst gradient is a ResBlock conv's, which this arithmetic
# leaves in fp32: the rerouted weight gradients move no class's worst error, the GEMM-form tensors' own errors stay below it.  The gates: 129
# flips on rows4112's 12.6 M feed-forward values, the farthest 7.4e-6 of max |x| from zero, on rows1380.)
EMULATED = dict(out=2.73e-5, loss=1.98e-7, stats=1.10e-5, running=3.82e-6, dx=5.63e-5, grad=1.12e-4, steps_loss=1.61e-5, steps_params=0.082)
BARS_X3W = {k: E.bar_of(EMULATED[k], E.FP32_BARS[k]) for k in EMULATED}
BARS_X3W["out"] = E.X3_OUT_BAR
assert EMULATED["out"] < 1e-4 and BARS_X3W["out"] < E.NORTH_STAR_TOL
# = out 2e-4, loss 1e-5, stats 4.4e-5, running 2e-5, dx 2.252e-4, grad 4.48e-4, steps_loss 1e-4, steps_params 0.328


def errors_x3w(got, ref):
    """O.errors with every quantity's bar replaced by its class's bf16x3w bar."""
    return {k: (e, BARS_X3W[k.split(".")[0]]) for k, (e, _) in O.errors(got, ref).items()}


if __name__ == "__main__":
    w, g = emulated_errors(verbose=True)
    print("EMULATED =", {k: float(f"{v:.3g}") for k, v in w.items()})
    print("largest gate gap", g)
