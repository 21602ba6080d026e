"""CPU emulation of the Transformer's bf16x3 arithmetic, to PREDICT its error before a GPU sees it ("bf16x3").

``Bf16x3Oracle`` is tests/transformer_oracle.py's float64 restatement with every GEMM of the forward — the six ResBlock convs and the 1 x 1
``residual_path`` (batch norms folded into their convs in double and rounded to fp32 first, as ``hificar_xfmr_finalize`` does), ``w_raw_in``,
q | k | v, ``w_o``, ``linear1``, ``linear2``, ``w_out`` — computed as

    x w  ~  hi(x) hi(w) + hi(x) lo(w) + lo(x) hi(w),      hi(a) = bf16(fp32(a)),  lo(a) = bf16(fp32(a) - hi(a))      (round to nearest even)

on operands split as the conv engine splits them, the three products summed in float64 (the device accumulates in fp32).  Everything that is
not a GEMM — attention, softmax, LayerNorm, bias and residual additions — stays float64.  So the difference from the float64 restatement
is the arithmetic's own error (the dropped lo lo term and the 16 bits a hi + lo pair keeps), without fp32 accumulation noise.

The emulation predicts; it is never what a device result is compared against.  Test infrastructure only.
"""

import torch
import torch.nn.functional as F

from transformer_oracle import TransformerOracle, banded_attention, dense_attention


def split(a):
    """(hi, lo) of ``a`` as float64 tensors holding bf16 values."""
    a32 = a.to(torch.float32)
    hi = a32.to(torch.bfloat16).to(torch.float32)
    lo = (a32 - hi).to(torch.bfloat16)
    return hi.to(torch.float64), lo.to(torch.float64)


def linear3(x, w, b=None):
    """F.linear(x, w, b) in bf16x3."""
    (xh, xl), (wh, wl) = split(x), split(w)
    y = F.linear(xh, wh) + F.linear(xh, wl) + F.linear(xl, wh)
    return y if b is None else y + b.to(torch.float32).to(torch.float64)


def conv3(x, w, b, padding):
    """F.conv1d(x, w, b, padding=padding) in bf16x3."""
    (xh, xl), (wh, wl) = split(x), split(w)
    y = F.conv1d(xh, wh, padding=padding) + F.conv1d(xh, wl, padding=padding) + F.conv1d(xl, wh, padding=padding)
    return y + b.to(torch.float32).to(torch.float64)[None, :, None]


class Bf16x3Oracle(TransformerOracle):
    def __init__(self, state_dict, dense=False, chunk=128):
        super().__init__(state_dict, dtype=torch.float64, device="cpu", dense=dense, chunk=chunk)

    def _folded(self, conv, bn):
        """Conv1d followed by an eval-mode BatchNorm1d as one conv, folded in double and rounded to fp32: (weight, bias)."""
        p = self.sd
        s = p[bn + ".weight"] / torch.sqrt(p[bn + ".running_var"] + 1e-5)
        w = (p[conv + ".weight"] * s[:, None, None]).to(torch.float32)
        b = ((p[conv + ".bias"] - p[bn + ".running_mean"]) * s + p[bn + ".bias"]).to(torch.float32)
        return w, b

    def _resblock(self, x, base):
        y = torch.relu(conv3(x, *self._folded(base + ".conv1", base + ".bn1"), padding=1))
        y = conv3(y, *self._folded(base + ".conv2", base + ".bn2"), padding=1)
        if base + ".residual_path.weight" in self.sd:
            x = conv3(x, *self._folded(base + ".residual_path", base + ".res_norm"), padding=0)
        return torch.relu(y + x)

    def attention(self, x, base):
        p = self.sd
        n, d = x.shape[-1], x.shape[-1] // 8
        # the q | k | v GEMM: row (h, a) of each weight is w[h, :, a]
        q, k, v = (linear3(x, p[f"{base}.{w}"].permute(0, 2, 1).reshape(n, n)).reshape(*x.shape[:2], 8, d).permute(0, 2, 1, 3)
                   for w in ("w_q", "w_k", "w_v"))
        emb = p[base + ".relative_positional.embeddings"][..., 0]
        o = dense_attention(q, k, v, emb) if self.dense else banded_attention(q, k, v, emb, self.chunk)
        # w_o's GEMM: row f of its weight is w_o[:, :, f] over (h, a)
        return linear3(o.permute(0, 2, 1, 3).reshape(*x.shape[:2], n), p[base + ".w_o"].reshape(n, n).t())

    @torch.no_grad()
    def forward(self, x, lengths=None, taps=None):
        if lengths is not None:
            return super().forward(x, lengths=lengths)  # (every utterance alone, through this method)
        x = torch.as_tensor(x).to(torch.float64)
        p = self.sd
        taps = taps if taps is not None else {}
        for i in range(3):
            x = self._resblock(x, f"conv_blocks.{i}")
        x = x.transpose(1, 2)
        taps["conv_blocks"] = x
        x = linear3(x, p["w_raw_in.weight"], p["w_raw_in.bias"])
        taps["w_raw_in"] = x
        n = x.shape[-1]
        for l in range(self.elayers):
            b = f"transformer.layers.{l}"
            x = F.layer_norm(x + self.attention(x, b + ".self_attn"), (n,), p[b + ".norm1.weight"], p[b + ".norm1.bias"], eps=1e-5)
            taps[f"layers.{l}.norm1"] = x
            y = linear3(torch.relu(linear3(x, p[b + ".linear1.weight"], p[b + ".linear1.bias"])), p[b + ".linear2.weight"], p[b + ".linear2.bias"])
            x = F.layer_norm(x + y, (n,), p[b + ".norm2.weight"], p[b + ".norm2.bias"], eps=1e-5)
            taps[f"layers.{l}"] = x
        return linear3(x, p["w_out.weight"], p["w_out.bias"]).transpose(1, 2)


# The models and inputs of tests/test_gpu_transformer_bf16x3.py that are not golden cases: (tag, constructor keywords, seed, input name, frames)
HEAD_CASES = tuple((f"hidden{h}", dict(in_channels=24, out_channels=40, elayers=1, hidden_dim=h), 6200 + h, "x.201", 201) for h in (256, 640, 1024))
WIDTH_CASES = (("in128_no_residual_path", dict(in_channels=128, out_channels=33, elayers=1, hidden_dim=128), 7301, "x.65", 65),
               ("in5_out33", dict(in_channels=5, out_channels=33, elayers=1, hidden_dim=128), 7302, "x.65", 65))


def emulated_errors():
    """{case: max|emulation - float64 restatement| / max|restatement|} on the exact inputs of the GPU tests (python tests/transformer_bf16x3_emulation.py)."""
    import os

    import numpy as np

    from conftest import GOLDEN, rel_err
    from articulatory_amd.utils.synth import synth_transformer_state_dict, uniform

    gold = np.load(os.path.join(GOLDEN, "gold_transformer.npz"))
    out = {}

    def run(tag, sd, x, lengths=None, taps=False):
        ta, tb = {}, {}
        a = Bf16x3Oracle(sd).forward(x, lengths=lengths, taps=ta)
        b = TransformerOracle(sd).forward(x, lengths=lengths, taps=tb)
        out[tag] = rel_err(a.numpy(), b.numpy())
        for name in (ta if taps else ()):
            out[f"{tag} tap {name}"] = rel_err(ta[name].numpy(), tb[name].numpy())

    for tag, frames in (("small", (1, 100, 101, 260)), ("default", (400,))):
        cin, cout, elayers, hidden, seed = (int(v) for v in gold[tag + "_params"])
        sd = synth_transformer_state_dict(dict(in_channels=cin, out_channels=cout, elayers=elayers, hidden_dim=hidden), seed=seed)
        for T in frames:
            run(f"{tag}_T{T}", sd, uniform(seed, f"x.{T}", (1, cin, T), -1.0, 1.0), taps=(tag == "small" and T == 260))
        if tag == "small":
            lens = [int(v) for v in gold["small_ragged_lengths"]]
            run("small_ragged", sd, uniform(seed, "ragged.x", (len(lens), cin, max(lens)), -1.0, 1.0), lengths=lens)
            run("small_inference", sd, uniform(seed, "inference.c", (200, cin), -2.0, 2.0).T[None])
    for tag, params, seed, name, T in HEAD_CASES + WIDTH_CASES:
        run(tag, synth_transformer_state_dict(params, seed=seed), uniform(seed, name, (1, params["in_channels"], T), -1.0, 1.0))
    return out


if __name__ == "__main__":
    import sys

    sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.abspath(__file__)))
    for case, err in emulated_errors().items():
        print(f"{case:40s} {err:.3g}")
