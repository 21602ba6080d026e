"""CPU emulation of the Transformer's bf16x3wa TRAINING arithmetic (``train_precision="bf16x3wa"``), to set the device's accuracy bars before a
GPU sees it ("bf16x3wa").

The bf16x3w emulation (tests/transformer_train_bf16x3w_emulation.py: its code, imported) with one more reroute, undone on exit:
``transformer_train_oracle.banded_attention_train`` — which both restatements call through the module — becomes a ``torch.autograd.Function``
that restates the arithmetic of the two query-tiled kernels.  With x ~ hi(x) + lo(x), hi = bf16(fp32(x)), lo = bf16(fp32(x) - hi), and
a b ~ hi hi + hi lo + lo hi ("a split product"):

    forward    S = (Q K^T) / sqrt(d) + gather(Q E^T)       two split products
               e = exp(S - max S), l = sum e               float64 (the device: fp32, the maximum per 64-key block)
               O = ((e o mask) V) / l                      e o mask (the dropout factor applied) and V split BEFORE the division by l
               L = max S + log l                           kept for the backward
    backward   S recomputed by the same statements, P = exp(S - L), Pd = P o mask
               dPd = dO V^T                                a split product
               Delta = dO . O,  dS = P o (dPd o mask - Delta)          float64 (the device: fp32)
               dQ = (dS K) / sqrt(d) + scatter(dS) E       two split products (dS split; the second sums over the table rows)
               dK = dS^T Q / sqrt(d),  dV = Pd^T dO,  dE = scatter(dS)^T Q     EXACT, from that dS and Pd: the key-tiled kernels stay fp32

Products and sums in float64 (the device accumulates in fp32, in another order: what the factor 4 is for).

The bars follow the project's rule, per class: E = the largest emulated error over every GPU case of
tests/test_gpu_transformer_train_bf16x3wa.py (DENSE_CASES, EDGE_CASES, the RAGGED_CASES, the five-step run) against the float64 restatement on
the emulation's own ReLU sides; the device bar is bf16x3w's where E is at most a quarter of it, otherwise 4 E; the output keeps 2e-4 while
E <= 5e-5.  EMULATED and BARS_X3WA below were recorded from ``python tests/transformer_train_bf16x3wa_emulation.py`` BEFORE the first GPU
run of the arithmetic; tests/test_transformer_train_bf16x3wa_host.py recomputes the errors and holds them to a quarter of the bars.  The
emulation predicts; the device is never compared against it.  Test infrastructure only.
"""

import contextlib

import torch

import transformer_ragged_oracle as R
import transformer_train_bf16x3_emulation as E
import transformer_train_bf16x3w_emulation as EW
import transformer_train_oracle as O
from transformer_bf16x3a_emulation import einsum3
from transformer_oracle import REL, _pos_index

DENSE_CASES = ("t2", "t65", "t101", "t200", "t263", "b1")              # of transformer_train_oracle.SHAPES: head size 16
EDGE_CASES = ("t330", "d32", "d48", "d64", "d80", "d112")              # of its EDGE_SHAPES
HEAD_CASES = ("d96", "d128")                                           # of SHAPES again: with EDGE_CASES, one per template instantiation
ALL_DENSE = DENSE_CASES + EDGE_CASES + HEAD_CASES
RAGGED_CASES = ("mixed", "tiles", "band", "zero")                      # of transformer_ragged_oracle.RAGGED_SHAPES: each padded and packed
TAB = 2 * REL - 1


def _chunks(T, chunk):
    for q0 in range(0, T, chunk):
        nq = min(chunk, T - q0)
        yield q0, nq, max(0, q0 - (REL - 1)), min(T, q0 + nq + (REL - 1))


def _logits(qc, kc, emb, rel, ok):
    """S of a query chunk against its key range, in split products; outside the band: -inf."""
    d = qc.shape[-1]
    s = einsum3("bhqa,bhka->bhqk", qc, kc) / (d ** 0.5)
    pos = einsum3("bhqa,hra->bhqr", qc, emb)
    s = s + torch.gather(pos, 3, rel.clamp(0, TAB - 1).expand(qc.shape[0], qc.shape[1], -1, -1))
    return s.masked_fill(~ok, float("-inf"))


class _Attention3(torch.autograd.Function):
    """banded_attention_train in the arithmetic of the module's docstring, its backward written out by hand."""

    @staticmethod
    def forward(ctx, q, k, v, emb, mask, chunk):
        B, H, T, d = q.shape
        out, lse = torch.empty_like(q), q.new_empty((B, H, T))
        for q0, nq, k0, k1 in _chunks(T, chunk):
            rel, ok = _pos_index(q0, nq, k0, k1 - k0, q.device)
            s = _logits(q[:, :, q0:q0 + nq], k[:, :, k0:k1], emb, rel, ok)
            m = s.max(dim=-1, keepdim=True).values
            e = torch.exp(s - m)  # (outside the band: exactly 0)
            l = e.sum(dim=-1, keepdim=True)
            if mask is not None:
                e = e * mask[:, :, q0:q0 + nq, k0:k1]
            out[:, :, q0:q0 + nq] = einsum3("bhqk,bhka->bhqa", e, v[:, :, k0:k1]) / l
            lse[:, :, q0:q0 + nq] = (m + torch.log(l))[..., 0]
        ctx.save_for_backward(q, k, v, emb, out, lse)
        ctx.mask, ctx.chunk = mask, chunk
        return out

    @staticmethod
    def backward(ctx, do):
        q, k, v, emb, out, lse = ctx.saved_tensors
        mask = ctx.mask
        B, H, T, d = q.shape
        dq, dk, dv, de = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v), torch.zeros_like(emb)
        delta = (do * out).sum(dim=-1, keepdim=True)
        for q0, nq, k0, k1 in _chunks(T, ctx.chunk):
            rel, ok = _pos_index(q0, nq, k0, k1 - k0, q.device)
            qc, kc, vc, doc = q[:, :, q0:q0 + nq], k[:, :, k0:k1], v[:, :, k0:k1], do[:, :, q0:q0 + nq]
            p = torch.exp(_logits(qc, kc, emb, rel, ok) - lse[:, :, q0:q0 + nq, None])  # (outside the band: exactly 0)
            dpd = einsum3("bhqa,bhka->bhqk", doc, vc)
            pd = p
            if mask is not None:
                mc = mask[:, :, q0:q0 + nq, k0:k1]
                pd, dpd = p * mc, dpd * mc
            ds = p * (dpd - delta[:, :, q0:q0 + nq])
            # dS by table row: (B, H, nq, 199), one more column collecting what lies outside the band (zeros)
            idx = torch.where(ok, rel, torch.full_like(rel, TAB)).expand(B, H, -1, -1)
            dsr = ds.new_zeros((B, H, nq, TAB + 1)).scatter_add(3, idx, ds)[..., :TAB]
            dq[:, :, q0:q0 + nq] = einsum3("bhqk,bhka->bhqa", ds, kc) / (d ** 0.5) + einsum3("bhqr,hra->bhqa", dsr, emb)
            dk[:, :, k0:k1] += torch.einsum("bhqk,bhqa->bhka", ds, qc) / (d ** 0.5)
            dv[:, :, k0:k1] += torch.einsum("bhqk,bhqa->bhka", pd, doc)
            de += torch.einsum("bhqr,bhqa->hra", dsr, qc)
        return dq, dk, dv, de, None, None


_attention = O.banded_attention_train  # (emulating() points O.banded_attention_train at attention3)


def attention3(q, k, v, emb, mask=None, chunk=128):
    return _Attention3.apply(q, k, v, emb, mask, chunk)


@contextlib.contextmanager
def emulating():
    """EW.emulating() with the attention of both restatements rerouted as well (they look it up in transformer_train_oracle when they run)."""
    with EW.emulating():
        O.banded_attention_train = attention3
        try:
            yield
        finally:
            O.banded_attention_train = _attention


def emulated_case(name):
    shapes = O.EDGE_SHAPES if name in O.EDGE_SHAPES else None
    with emulating():
        emu = O.restatement(name, torch.float64, shapes=shapes)
    return emu, O.restatement(name, torch.float64, gates=emu["sides"], shapes=shapes)


def emulated_ragged(name):
    """E.emulated_ragged's statements for any RAGGED_SHAPES entry, under this module's reroute."""
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


def emulated_errors(verbose=False, cases=ALL_DENSE, ragged=RAGGED_CASES, steps=True):
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


def bar_of(emulated, x3w_bar):
    """The device bar of a class: bf16x3w's where the emulated error is at most a quarter of it, otherwise 4 E."""
    return x3w_bar if emulated <= x3w_bar / 4 else 4 * emulated


# ---- recorded before the first GPU run (see the module's docstring); E: emulated (rounded up in its third digit), bar: what the device is held to
# (The worst cases: out t65; loss b1; stats, running and grad t2; dx t200.  Against bf16x3w's E — out 2.73e-5, dx 5.63e-5, grad 1.12e-4 — the
# attention's split products move out, dx and grad a little: dx and grad now lie above a quarter of bf16x3w's bars, so theirs are 4 E.  The
# gates: 19 flips on t263, the farthest 9.9e-6 of max |x| from zero, on `tiles`.)
EMULATED = dict(out=2.91e-5, loss=1.49e-7, stats=1.10e-5, running=3.82e-6, dx=6.00e-5, grad=1.25e-4, steps_loss=1.74e-5, steps_params=0.082)
BARS_X3WA = {k: bar_of(EMULATED[k], EW.BARS_X3W[k]) for k in EMULATED}
BARS_X3WA["out"] = E.X3_OUT_BAR if EMULATED["out"] <= 5e-5 else 4 * EMULATED["out"]
assert BARS_X3WA["out"] < E.NORTH_STAR_TOL
# = out 2e-4, loss 1e-5, stats 4.4e-5, running 2e-5, dx 2.4e-4, grad 5e-4, steps_loss 1e-4, steps_params 0.328


def errors_x3wa(got, ref):
    """O.errors with every quantity's bar replaced by its class's bf16x3wa bar."""
    return {k: (e, BARS_X3WA[k.split(".")[0]]) for k, (e, _) in O.errors(got, ref).items()}


if __name__ == "__main__":
    w, g = emulated_errors(verbose=True)
    print("EMULATED =", {k: float(f"{v:.3g}") for k, v in w.items()})
    print("largest gate gap", g)
