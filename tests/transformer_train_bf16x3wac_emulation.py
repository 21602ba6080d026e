"""CPU emulation of the Transformer's bf16x3wac TRAINING arithmetic (``train_precision="bf16x3wac"``), to set the device's accuracy bars before a
GPU sees it ("bf16x3wac").

The bf16x3wa emulation (tests/transformer_train_bf16x3wa_emulation.py: its code, imported) with one more reroute, undone on exit: the weight
gradient of every k = 3 conv the device's rule selects (``gemm3_form``: three taps, at least four 32-blocks of output channels and of input
columns, 3 cin_pad <= 3072 — ``conv_blocks.{1,2}.conv1``, ``conv_blocks.{0,1,2}.conv2``, and ``conv_blocks.0.conv1`` where the input is that
wide) is, tap by tap,

    dW[:, :, k] = G^T A_k ~ hi(G)^T hi(A_k) + hi(G)^T lo(A_k) + lo(G)^T hi(A_k)      A_k[b, t] = A[b, t + k - 1], zero outside the sequence

with hi(a) = bf16(fp32(a)), lo(a) = bf16(fp32(a) - hi(a)) — the device's one GEMM over the columns k cin_pad + c is these three products side by
side — and the bias gradient of such a layer is the sum over the rows of hi(G) + lo(G), which is what wgrad_bf16x3_kernel sums from the G tile it
has staged.  The forward and the data gradient of these convs are bf16x3's own statements (E.conv3's, one product per tap), so nothing but
these tensors moves.  Products and sums in float64 (the device accumulates in fp32, in another order: what the factor 4 is for).

The bars follow the project's rule, per class: E = the largest emulated error over every GPU case of
tests/test_gpu_transformer_train_bf16x3wac.py (CASES, EDGE_CASES, EXTRA_CASES, the RAGGED_CASES, the five-step run) against the float64 restatement on the
emulation's own ReLU sides; the device bar is bf16x3wa's where E is at most a quarter of it, otherwise 4 E; the output keeps 2e-4.  EMULATED
and BARS_X3WAC below were recorded from ``python tests/transformer_train_bf16x3wac_emulation.py`` BEFORE the first GPU run of the arithmetic;
tests/test_transformer_train_bf16x3wac_host.py recomputes the errors and holds them to a quarter of the bars.  The emulation predicts; the
device is never compared against it.  Test infrastructure only.
"""

import contextlib

import torch
import torch.nn.functional as F

import transformer_bf16x3wac_forms as WC
import transformer_ragged_oracle as R
import transformer_train_bf16x3_emulation as E
import transformer_train_bf16x3w_emulation as EW
import transformer_train_bf16x3wa_emulation as EWA
import transformer_train_oracle as O
from transformer_bf16x3_emulation import split

CASES = ("t2", "t65", "nores")                  # of transformer_train_oracle.SHAPES: what tests/test_gpu_transformer_train_bf16x3wac.py runs
EDGE_CASES = ("d48", "rows1380", "rows4112")    # ... and of its EDGE_SHAPES
EXTRA_CASES = ("pad101",)                       # ... and of transformer_bf16x3wac_forms.EXTRA_SHAPES: conv_blocks.0.conv1 moves with cin_pad != cin
RAGGED_CASES = ("mixed", "nores")               # of transformer_ragged_oracle.RAGGED_SHAPES: each padded and packed on the device


def gemm3_form(cout, cin, K):
    """wgrad_gemm3_form (hificar_xfmr_train.hip.inc) of a (cout, cin, K) weight whose input rows are padded to a multiple of 32 columns."""
    pad = (cin + 31) // 32 * 32
    return K == 3 and (cout + 31) // 32 >= 4 and pad >= 128 and 3 * pad <= 3072


class _AddBiasW(torch.autograd.Function):
    """y (B, N, T) + b; the bias gradient as the sum over the rows of hi(G) + lo(G)."""

    @staticmethod
    def forward(ctx, y, b):
        return y + b[None, :, None]

    @staticmethod
    def backward(ctx, dy):
        gh, gl = split(dy.transpose(1, 2).reshape(-1, dy.shape[1]))
        return dy, (gh + gl).sum(0)


def conv3wac(x, w, b=None, padding=0):
    """E.conv3 — the same forward, the same data gradient — with, for a layer gemm3_form selects, each tap's weight gradient in bf16x3 on the
    tap-shifted rows (EW._Linear3W's backward) and the bias gradient from the split rows."""
    if not gemm3_form(*w.shape):
        return EW.conv3w(x, w, b, padding)
    T, xp = x.shape[2], F.pad(x, (padding, padding))
    y = sum(EW._Linear3W.apply(xp[:, :, k:k + T].transpose(1, 2), w[:, :, k], None) for k in range(w.shape[2])).transpose(1, 2)
    return y if b is None else _AddBiasW.apply(y, b)


class _FWAC(EW._FW):
    conv1d = staticmethod(conv3wac)


@contextlib.contextmanager
def emulating():
    """EWA.emulating() with the selected convs' weight and bias gradients rerouted as well."""
    with EWA.emulating():
        before = O.F
        O.F = R.F = _FWAC()
        try:
            yield
        finally:
            O.F = R.F = before


def emulated_case(name):
    shapes = WC.case_shapes(name)
    with emulating():
        emu = O.restatement(name, torch.float64, shapes=shapes)
    return emu, O.restatement(name, torch.float64, gates=emu["sides"], shapes=shapes)


def emulated_ragged(name):
    """EWA.emulated_ragged's statements under this module's reroute."""
    class Sides(R.TransformerRaggedOracle):
        def _relu_v(self, x, name, v):
            self.sides[name] = (x > 0) & v.expand_as(x)
            return super()._relu_v(x, name, v)

    params, sd, x, t, lengths = R.ragged_case(name)
    with emulating():
        o = Sides(sd, dtype=torch.float64, dropout=params["dropout"], seed=O.DROPOUT_SEED)
        emu = o.step_padded(x, t, lengths)
        emu["running"] = dict(o.buffers)
    return emu, R.ragged_restatement(name, torch.float64, gates=o.sides)


def emulated_errors(verbose=False, cases=CASES + EDGE_CASES + EXTRA_CASES, ragged=RAGGED_CASES, steps=True):
    """{class: largest emulated error over the cases}, the five-step run's as "steps_loss" / "steps_params"; and the largest gate gap."""
    worst, gap = {}, 0.0
    runs = [(name, emulated_case) for name in cases] + [(name, emulated_ragged) for name in ragged]
    for name, fn in runs:
        emu, ref = fn(name)
        c = E.classes(O.errors(emu, ref))
        gap = max(gap, ref["gate_gap"])
        if verbose:
            print(f"{name}: {ref['gate_flips']} flips, gap {ref['gate_gap']:.3g}; " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(c.items())), flush=True)
        for k, v in c.items():
            worst[k] = max(worst.get(k, 0.0), v)
    if steps:
        with emulating():
            losses, final = O.five_steps(torch.float64)
        e_loss, per = O.five_step_errors(losses, final, *O.five_steps(torch.float64))
        worst["steps_loss"], worst["steps_params"] = e_loss, max(per.values())
        if verbose:
            print(f"five steps: loss {e_loss:.3g}, parameters {max(per.values()):.3g} ({max(per, key=per.get)})")
    return worst, gap


# ---- recorded before the first GPU run (see the module's docstring); E: emulated (rounded up in its third digit), bar: what the device is held to
# (The worst cases: out t65; loss the ragged nores; stats, running, dx and grad t2.  The forward and the data gradients are bf16x3wa's, so only
# grad can move against its E: at t2's 4 rows conv_blocks.1.conv1.weight goes from 1.24e-4 to 1.29e-4, which is above a quarter of bf16x3wa's
# 5e-4, so the gradient bar is 4 E.  The bias gradients' split sums are not what moves it: with exact bias sums the emulation gives the same
# worst tensors and the same figures, so the biases stay on the staged G tile's sums.  The gates: 136 flips on rows4112, the farthest 6.9e-6 of
# max |x| from zero, on rows1380.)
EMULATED = dict(out=2.91e-5, loss=2.06e-7, stats=1.10e-5, running=3.82e-6, dx=5.64e-5, grad=1.30e-4, steps_loss=1.60e-5, steps_params=0.081)
BARS_X3WAC = {k: EWA.bar_of(EMULATED[k], EWA.BARS_X3WA[k]) for k in EMULATED}
BARS_X3WAC["out"] = E.X3_OUT_BAR
assert EMULATED["out"] < 1e-4 and BARS_X3WAC["out"] < E.NORTH_STAR_TOL
# = out 2e-4, loss 1e-5, stats 4.4e-5, running 2e-5, dx 2.4e-4, grad 5.2e-4, steps_loss 1e-4, steps_params 0.328


def errors_x3wac(got, ref):
    """O.errors with every quantity's bar replaced by its class's bf16x3wac bar."""
    return {k: (e, BARS_X3WAC[k.split(".")[0]]) for k, (e, _) in O.errors(got, ref).items()}


if __name__ == "__main__":
    w, g = emulated_errors(verbose=True)
    print("EMULATED =", {k: float(f"{v:.3g}") for k, v in w.items()})
    print("largest gate gap", g)
