"""CPU emulation of the Transformer's bf16x3wack TRAINING arithmetic (``train_precision="bf16x3wack"``), to set the device's accuracy bars before
a GPU sees it ("bf16x3wack").

The bf16x3wac emulation (tests/transformer_train_bf16x3wac_emulation.py: its code, imported, none of it changed) with one more reroute, undone
on exit: ``transformer_train_oracle.banded_attention_train`` becomes the bf16x3wa emulation's attention with the last line of its backward
restated.  The three products the key-tiled kernels compute are split products of the emulation's own dS, Pd, Q and dO (x ~ hi(x) + lo(x),
hi = bf16(fp32(x)), lo = bf16(fp32(x) - hi), a b ~ hi hi + hi lo + lo hi):

    dK = dS^T Q / sqrt(d),  dV = Pd^T dO,  dE = scatter(dS)^T Q        split products (bf16x3wa, bf16x3wac: exact)

The forward, L, Delta, dS, Pd and dQ are bf16x3wa's statements, untouched: out, loss, statistics and the last layer's dQ cannot move.
Products and sums in float64 (the device accumulates in fp32, in another order: what the factor 4 is for).

The bars follow the project's rule, per class: E = the largest emulated error over every GPU case of
tests/test_gpu_transformer_train_bf16x3wack.py (DENSE_CASES, HEAD_CASES, the RAGGED_CASES, the five-step run) against the float64 restatement
on the emulation's own ReLU sides; the device bar is bf16x3wac's where E is at most a quarter of it, otherwise 4 E; the output keeps 2e-4.
EMULATED and BARS_X3WACK below were recorded from ``python tests/transformer_train_bf16x3wack_emulation.py`` BEFORE the first GPU run of the
arithmetic; tests/test_transformer_train_bf16x3wack_host.py recomputes the errors and holds them to a quarter of the bars.  The emulation
predicts; the device is never compared against it.  Test infrastructure only.
"""

import contextlib

import torch

import transformer_bf16x3wac_forms as WC
import transformer_ragged_oracle as R
import transformer_train_bf16x3_emulation as E
import transformer_train_bf16x3wa_emulation as EWA
import transformer_train_bf16x3wac_emulation as EC
import transformer_train_oracle as O
from transformer_bf16x3a_emulation import einsum3
from transformer_oracle import _pos_index

DENSE_CASES = ("t2", "t65", "t101", "t200", "t263", "b1", "t330")      # head size 16 at the tile and band edges (t330: of EDGE_SHAPES)
HEAD_CASES = ("d32", "d48", "d64", "d80", "d96", "d112", "d128")       # one per template instantiation
ALL_DENSE = DENSE_CASES + HEAD_CASES
RAGGED_CASES = ("mixed", "tiles", "band", "zero")                      # of transformer_ragged_oracle.RAGGED_SHAPES: each padded and packed
TAB = EWA.TAB


class _Attention3K(EWA._Attention3):
    """EWA._Attention3 — the same forward (inherited), the same statements for dS, Pd and dQ — with dK, dV and dE as split products."""

    @staticmethod
    def backward(ctx, do):
        q, k, v, emb, out, lse = ctx.saved_tensors
        mask = ctx.mask
        B, H, T, d = q.shape
        dq, dk, dv, de = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v), torch.zeros_like(emb)
        delta = (do * out).sum(dim=-1, keepdim=True)
        for q0, nq, k0, k1 in EWA._chunks(T, ctx.chunk):
            rel, ok = _pos_index(q0, nq, k0, k1 - k0, q.device)
            qc, kc, vc, doc = q[:, :, q0:q0 + nq], k[:, :, k0:k1], v[:, :, k0:k1], do[:, :, q0:q0 + nq]
            p = torch.exp(EWA._logits(qc, kc, emb, rel, ok) - lse[:, :, q0:q0 + nq, None])  # (outside the band: exactly 0)
            dpd = einsum3("bhqa,bhka->bhqk", doc, vc)
            pd = p
            if mask is not None:
                mc = mask[:, :, q0:q0 + nq, k0:k1]
                pd, dpd = p * mc, dpd * mc
            ds = p * (dpd - delta[:, :, q0:q0 + nq])
            idx = torch.where(ok, rel, torch.full_like(rel, TAB)).expand(B, H, -1, -1)
            dsr = ds.new_zeros((B, H, nq, TAB + 1)).scatter_add(3, idx, ds)[..., :TAB]
            dq[:, :, q0:q0 + nq] = einsum3("bhqk,bhka->bhqa", ds, kc) / (d ** 0.5) + einsum3("bhqr,hra->bhqa", dsr, emb)
            # the key-tiled kernels: the split of a value does not depend on the block it is met in, so the chunks' shares add up
            dk[:, :, k0:k1] += einsum3("bhqk,bhqa->bhka", ds, qc) / (d ** 0.5)
            dv[:, :, k0:k1] += einsum3("bhqk,bhqa->bhka", pd, doc)
            de += einsum3("bhqr,bhqa->hra", dsr, qc)
        return dq, dk, dv, de, None, None


def attention3k(q, k, v, emb, mask=None, chunk=128):
    return _Attention3K.apply(q, k, v, emb, mask, chunk)


@contextlib.contextmanager
def emulating():
    """EC.emulating() with the attention's backward rerouted as well; on exit the attention is whatever it was on entry."""
    with EC.emulating():
        before = O.banded_attention_train
        O.banded_attention_train = attention3k
        try:
            yield
        finally:
            O.banded_attention_train = before


def emulated_case(name):
    shapes = WC.case_shapes(name)
    with emulating():
        emu = O.restatement(name, torch.float64, shapes=shapes)
    return emu, O.restatement(name, torch.float64, gates=emu["sides"], shapes=shapes)


def emulated_ragged(name):
    """EC.emulated_ragged's statements under this module's reroute."""
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


# ---- recorded before the first GPU run (see the module's docstring); E: emulated (rounded up in its third digit), bar: what the device is held to
# (The worst cases: out t65; loss b1; stats, running and grad t2; dx t200.  The cases are bf16x3wa's, not bf16x3wac's — they share t2, t65 and
# d48 — so the figures are not to be read one by one against bf16x3wac's E.  The forward is untouched: out, loss, stats and running are bf16x3wa's
# figures on these cases.  Every class lies within a quarter of bf16x3wac's bar, so every bar is bf16x3wac's.  The gates: 19 flips on t263, the
# farthest 9.9e-6 of max |x| from zero, on `tiles`.)
EMULATED = dict(out=2.91e-5, loss=1.49e-7, stats=1.10e-5, running=3.82e-6, dx=5.32e-5, grad=1.18e-4, steps_loss=1.32e-5, steps_params=0.0811)
BARS_X3WACK = {k: EWA.bar_of(EMULATED[k], EC.BARS_X3WAC[k]) for k in EMULATED}
BARS_X3WACK["out"] = E.X3_OUT_BAR
assert EMULATED["out"] < 1e-4 and BARS_X3WACK["out"] < E.NORTH_STAR_TOL
# = out 2e-4, loss 1e-5, stats 4.4e-5, running 2e-5, dx 2.4e-4, grad 5.2e-4, steps_loss 1e-4, steps_params 0.328: bf16x3wac's, all of them


def errors_x3wack(got, ref):
    """O.errors with every quantity's bar replaced by its class's bf16x3wack bar."""
    return {k: (e, BARS_X3WACK[k.split(".")[0]]) for k, (e, _) in O.errors(got, ref).items()}


if __name__ == "__main__":
    w, g = emulated_errors(verbose=True)
    print("EMULATED =", {k: float(f"{v:.3g}") for k, v in w.items()})
    print("largest gate gap", g)
