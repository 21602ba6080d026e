"""CPU emulation of the Transformer's bf16x3 TRAINING arithmetic (``train_precision="bf16x3"``), to set the device's accuracy bars before a
GPU sees it ("bf16x3 training").

``emulating()`` runs the float64 training restatements (tests/transformer_train_oracle.py, tests/transformer_ragged_oracle.py) — their own
code — with the GEMM calls rerouted:

    forward        every GEMM (the six ResBlock convs and ``residual_path``, ``w_raw_in``, q | k | v, ``w_o``, ``linear1``, ``linear2``, ``w_out``) is
                   x w ~ hi(x) hi(w) + hi(x) lo(w) + lo(x) hi(w),   hi(a) = bf16(fp32(a)),  lo(a) = bf16(fp32(a) - hi(a))   (round to nearest even)
    data gradient  the same expression on the split output gradient and the split weight (a custom autograd function)
    weight, bias   gradients exact
    the rest       attention, softmax, norms, dropout, additions: float64 as they stand

with the three products summed in float64 (the device accumulates in fp32 and sums rows in another order: what the factor 4 below is for).

The bars.  For every quantity the fp32 suite bounds, E = the largest emulated error over the GPU cases (CASES, RAGGED_CASE, the five-step run)
against the float64 restatement run with the emulation's ReLU sides (``gates=``).  The device bar is the fp32 bar where E is at most a quarter
of it, otherwise 4 E; the output keeps the project's precedent (emulated < 1e-4 -> bar 2e-4).  EMULATED and BARS_X3 below were recorded from
``python tests/transformer_train_bf16x3_emulation.py`` before the first GPU run; tests/test_transformer_train_bf16x3_host.py recomputes the
errors and holds them to a quarter of the bars.  The emulation predicts; the device is never compared against it.  Test infrastructure only.
"""

import contextlib

import torch
import torch.nn.functional as F

import transformer_ragged_oracle as R
import transformer_train_oracle as O
from transformer_bf16x3_emulation import split

CASES = ("t2", "t65", "t101", "t263", "d96", "nores")  # of transformer_train_oracle.SHAPES: what tests/test_gpu_transformer_train_bf16x3.py runs
RAGGED_CASE = "mixed"                                  # of transformer_ragged_oracle.RAGGED_SHAPES: B = 3, T = 70, lengths (70, 33, 1)
NORTH_STAR_TOL = 1e-3
X3_OUT_BAR = 2e-4                                      # the bf16x3 output bar (tests/test_gpu_transformer_bf16x3.py), also the gate-flip gap


def mm3(a, b):
    """a @ b in bf16x3: a (..., K), b (K, N)."""
    (ah, al), (bh, bl) = split(a), split(b)
    return ah @ bh + ah @ bl + al @ bh


class _Linear3(torch.autograd.Function):
    """x (..., K), w (N, K) -> x w^T in bf16x3; the data gradient in bf16x3 on the split output gradient, the weight gradient exact."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return mm3(x, w.t())

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        return mm3(dy, w), dy.reshape(-1, dy.shape[-1]).t() @ x.reshape(-1, x.shape[-1])


def linear3(x, w, b=None):
    y = _Linear3.apply(x, w)
    return y if b is None else y + b


def conv3(x, w, b=None, padding=0):
    """F.conv1d (stride 1, odd kernel) as one bf16x3 product per tap: (B, C, T) -> (B, N, T)."""
    T, xp = x.shape[2], F.pad(x, (padding, padding))
    y = sum(_Linear3.apply(xp[:, :, k:k + T].transpose(1, 2), w[:, :, k]) for k in range(w.shape[2])).transpose(1, 2)
    return y if b is None else y + b[None, :, None]


class _F:
    """torch.nn.functional with linear and conv1d in bf16x3."""
    linear, conv1d = staticmethod(linear3), staticmethod(conv3)

    def __getattr__(self, name):
        return getattr(F, name)


def _einsum3(real):
    def einsum(eq, *ops):
        if eq == "btf,hfa->bhta":  # q, k or v: row (h, a) of the GEMM's weight is w[h, :, a]
            x, w = ops
            H, n, A = w.shape
            return linear3(x, w.permute(0, 2, 1).reshape(H * A, n)).view(x.shape[0], x.shape[1], H, A).permute(0, 2, 1, 3)
        if eq == "bhta,haf->btf":  # w_o
            o, w = ops
            H, A, n = w.shape
            return linear3(o.permute(0, 2, 1, 3).reshape(o.shape[0], o.shape[2], H * A), w.reshape(H * A, n).t())
        return real(eq, *ops)
    return einsum


@contextlib.contextmanager
def emulating():
    """Inside: the restatements' F.linear, F.conv1d and their two projection einsums compute in bf16x3 (the attention's einsums do not)."""
    real = torch.einsum
    O.F = R.F = _F()
    torch.einsum = _einsum3(real)
    try:
        yield
    finally:
        O.F = R.F = F
        torch.einsum = real


def emulated_case(name):
    """(the emulation's step on a SHAPES entry, the float64 restatement's on the emulation's ReLU sides)."""
    with emulating():
        emu = O.restatement(name, torch.float64)
    return emu, O.restatement(name, torch.float64, gates=emu["sides"])


def emulated_ragged():
    """The same for RAGGED_CASE.  The ragged restatement records no sides; a run with float64's own gates records, through gate_gap, how
    far from zero the farthest ReLU input lies that the emulation took on the other side."""
    class Sides(R.TransformerRaggedOracle):
        def _relu_v(self, x, name, v):
            self.sides[name] = (x > 0) & v.expand_as(x)
            return super()._relu_v(x, name, v)

    params, sd, x, t, lengths = R.ragged_case(RAGGED_CASE)
    with emulating():
        o = Sides(sd, dtype=torch.float64, dropout=params["dropout"], seed=O.DROPOUT_SEED)
        emu = o.step_padded(x, t, lengths)
        emu["running"] = dict(o.buffers)
    ref = R.ragged_restatement(RAGGED_CASE, torch.float64, gates=o.sides)
    return emu, ref


def classes(errs):
    """O.errors' {quantity: (error, fp32 bar)} -> {class: largest error}: out, loss, stats, running, dx, grad."""
    out = {}
    for k, (e, _) in errs.items():
        c = k.split(".")[0]
        out[c] = max(out.get(c, 0.0), e)
    return out


def emulated_errors(verbose=False):
    """{class: largest emulated error over the cases}, the five-step run's as "steps_loss" / "steps_params"; and the largest gate gap."""
    worst, gap = {}, 0.0
    runs = [(name, emulated_case) for name in CASES] + [(RAGGED_CASE + " (ragged)", lambda _: emulated_ragged())]
    for name, fn in runs:
        emu, ref = fn(name)
        c = classes(O.errors(emu, ref))
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


def bar_of(emulated, fp32_bar):
    return fp32_bar if emulated <= fp32_bar / 4 else 4 * emulated


# ---- recorded before the first GPU run (see the module's docstring); E: emulated, bar: what the device is held to
# (E rounded up in its third digit.  The worst cases: out t65, loss / stats / running / dx / grad t2, the gates: 19 flips on t263, the farthest
# 5.1e-6 of max |x| from zero.)
EMULATED = dict(out=2.73e-5, loss=1.98e-7, stats=1.10e-5, running=3.82e-6, dx=5.63e-5, grad=1.12e-4, steps_loss=1.65e-5, steps_params=0.082)
FP32_BARS = dict(out=O.BARS["out"], loss=O.BARS["loss"], stats=O.BARS["out"], running=O.BARS["out"], dx=O.BARS["grad"], grad=O.BARS["grad"],
                 steps_loss=1e-4,      # tests/test_gpu_transformer_train.py: the five-step run's loss bar
                 steps_params=0.0)     # the fp32 suite prints the final parameters and bounds nothing (Adam's lr g / (|g| + eps) on elements whose
                                       # gradient is rounding noise): no fp32 bar to keep, so 4 E — a bar that says little, as E = 0.082 of a
                                       # tensor's max shows; the loss bar and the eval check are what hold the run
BARS_X3 = {k: bar_of(EMULATED[k], FP32_BARS[k]) for k in EMULATED}
BARS_X3["out"] = X3_OUT_BAR            # emulated < 1e-4: the project's bf16x3 output bar
assert EMULATED["out"] < 1e-4 and BARS_X3["out"] < NORTH_STAR_TOL
# = out 2e-4, loss 1e-5, stats 4.4e-5, running 2e-5, dx 2.252e-4, grad 4.48e-4, steps_loss 1e-4, steps_params 0.328


def errors_x3(got, ref):
    """O.errors with every quantity's bar replaced by its class's bf16x3 bar."""
    return {k: (e, BARS_X3[k.split(".")[0]]) for k, (e, _) in O.errors(got, ref).items()}


if __name__ == "__main__":
    w, g = emulated_errors(verbose=True)
    print("EMULATED =", {k: float(f"{v:.3g}") for k, v in w.items()})
    print("largest gate gap", g)
