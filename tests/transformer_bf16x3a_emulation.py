"""CPU emulation of the Transformer's bf16x3a arithmetic, to PREDICT its error before a GPU sees it ("bf16x3a").

``Bf16x3aOracle`` is ``Bf16x3Oracle`` (every GEMM as hi hi + hi lo + lo hi) with the attention's three products in the same arithmetic:

    S = (Q K^T) / sqrt(d) + Q E^T      Q, K, E split, each product as three split products
    P = exp(S - max S)                 float64; split BEFORE the division by the row sum, as the kernel splits it
    O = (P V) / sum P                  P and V split, three split products

the three products summed in float64 (the device accumulates in fp32, and takes its maximum per 64-key block).  Softmax, LayerNorm and the
additions stay float64.  ``python tests/transformer_bf16x3a_emulation.py`` prints the table of DESIGN.md.

The emulation predicts; it is never what a device result is compared against.  Test infrastructure only.
"""

import torch

from transformer_bf16x3_emulation import HEAD_CASES, WIDTH_CASES, Bf16x3Oracle, split
from transformer_oracle import REL, _pos_index

# hidden sizes of the one-layer models that cover the attention kernel's eight head sizes 16 .. 128 (T = 201)
ALL_HEAD_CASES = tuple((f"hidden{h}", dict(in_channels=24, out_channels=40, elayers=1, hidden_dim=h), 6200 + h, "x.201", 201)
                       for h in (128, 256, 384, 512, 640, 768, 896, 1024))
PEAKED_GAIN = 4.0  # the "peaked softmax" input: the small golden model with every self_attn.w_q multiplied by this, T = 260


def einsum3(eq, a, b):
    """torch.einsum(eq, a, b) in bf16x3."""
    (ah, al), (bh, bl) = split(a), split(b)
    return torch.einsum(eq, ah, bh) + torch.einsum(eq, ah, bl) + torch.einsum(eq, al, bh)


def banded_attention3(q, k, v, emb, chunk=128, stats=None):
    """transformer_oracle.banded_attention with its three products in bf16x3.  stats (a dict): max |logit| and the mean top probability."""
    B, H, T, d = q.shape
    out = torch.empty_like(q)
    for q0 in range(0, T, chunk):
        nq = min(chunk, T - q0)
        k0, k1 = max(0, q0 - (REL - 1)), min(T, q0 + nq + (REL - 1))
        qc = q[:, :, q0:q0 + nq]
        s = einsum3("bhqa,bhka->bhqk", qc, k[:, :, k0:k1]) / (d ** 0.5)
        rel, ok = _pos_index(q0, nq, k0, k1 - k0, q.device)
        pos = einsum3("bhqa,hra->bhqr", qc, emb)
        s = s + torch.gather(pos, 3, rel.clamp(0, 2 * REL - 2).expand(B, H, -1, -1))
        s = s.masked_fill(~ok, float("-inf"))
        e = torch.exp(s - s.max(dim=-1, keepdim=True).values)  # (outside the band: exactly 0)
        l = e.sum(dim=-1, keepdim=True)
        out[:, :, q0:q0 + nq] = einsum3("bhqk,bhka->bhqa", e, v[:, :, k0:k1]) / l
        if stats is not None:
            stats["max_abs_logit"] = max(stats.get("max_abs_logit", 0.0), float(s[ok.expand_as(s)].abs().max()))
            stats.setdefault("top", []).append((e / l).max(dim=-1).values.flatten())
    return out


class Bf16x3aOracle(Bf16x3Oracle):
    def __init__(self, state_dict, chunk=128):
        super().__init__(state_dict, dense=False, chunk=chunk)
        self.stats = {}

    def attention(self, x, base):
        from transformer_bf16x3_emulation import linear3

        p = self.sd
        n, d = x.shape[-1], x.shape[-1] // 8
        q, k, v = (linear3(x, p[f"{base}.{w}"].permute(0, 2, 1).reshape(n, n)).reshape(*x.shape[:2], 8, d).permute(0, 2, 1, 3)
                   for w in ("w_q", "w_k", "w_v"))
        o = banded_attention3(q, k, v, p[base + ".relative_positional.embeddings"][..., 0], self.chunk, self.stats)
        return linear3(o.permute(0, 2, 1, 3).reshape(*x.shape[:2], n), p[base + ".w_o"].reshape(n, n).t())


def peaked_state_dict(sd, gain=PEAKED_GAIN):
    """sd with every self_attn.w_q multiplied by gain: logits and their sensitivity to operand error grow with it."""
    import numpy as np

    return {k: (np.asarray(v) * np.float32(gain) if k.endswith("self_attn.w_q") else v) for k, v in sd.items()}


def emulated_errors(gains=(PEAKED_GAIN,)):
    """{case: (bf16x3 error, bf16x3a error, max|bf16x3a - bf16x3|, max |logit|, mean top probability)}, errors as max|. - float64
    restatement| / max|restatement|, on the exact inputs of tests/test_gpu_transformer_bf16x3a.py."""
    import os

    import numpy as np

    from conftest import GOLDEN, rel_err
    from transformer_oracle import TransformerOracle
    from articulatory_amd.utils.synth import synth_transformer_state_dict, uniform

    gold = np.load(os.path.join(GOLDEN, "gold_transformer.npz"))
    out = {}

    def run(tag, sd, x, lengths=None):
        oa = Bf16x3aOracle(sd)
        a = oa.forward(x, lengths=lengths).numpy()
        b = Bf16x3Oracle(sd).forward(x, lengths=lengths).numpy()
        r = TransformerOracle(sd).forward(x, lengths=lengths).numpy()
        scale = float(np.abs(r).max())
        out[tag] = (rel_err(b, r), rel_err(a, r), float(np.abs(a - b).max()) / scale, oa.stats["max_abs_logit"], float(torch.cat(oa.stats["top"]).mean()))

    for tag, frames in (("small", (1, 100, 101, 260)), ("default", (400,))):
        cin, cout, elayers, hidden, seed = (int(v) for v in gold[tag + "_params"])
        sd = synth_transformer_state_dict(dict(in_channels=cin, out_channels=cout, elayers=elayers, hidden_dim=hidden), seed=seed)
        for T in frames:
            run(f"{tag}_T{T}", sd, uniform(seed, f"x.{T}", (1, cin, T), -1.0, 1.0))
        if tag == "small":
            lens = [int(v) for v in gold["small_ragged_lengths"]]
            run("small_ragged", sd, uniform(seed, "ragged.x", (len(lens), cin, max(lens)), -1.0, 1.0), lengths=lens)
            run("small_inference", sd, uniform(seed, "inference.c", (200, cin), -2.0, 2.0).T[None])
            for gain in gains:
                run(f"small_T260_wq_gain{gain:g}", peaked_state_dict(sd, gain), uniform(seed, "x.260", (1, cin, 260), -1.0, 1.0))
    for tag, params, seed, name, T in ALL_HEAD_CASES + WIDTH_CASES:
        run(tag, synth_transformer_state_dict(params, seed=seed), uniform(seed, name, (1, params["in_channels"], T), -1.0, 1.0))
    return out


if __name__ == "__main__":
    import sys

    sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.abspath(__file__)))
    print(f"{'case':32s} {'bf16x3':>9s} {'bf16x3a':>9s} {'a - x3':>9s} {'max|s|':>7s} {'mean top p':>10s}")
    for case, (e3, ea, dd, ms, tp) in emulated_errors(gains=(4.0, 16.0, 64.0)).items():
        print(f"{case:32s} {e3:9.3g} {ea:9.3g} {dd:9.3g} {ms:7.3g} {tp:10.3g}")
