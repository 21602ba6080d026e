#!/usr/bin/env python3
"""Device time of the native WavLM encoder (articulatory_amd.features.WavLM, the large model: 24 x 1024, conv 512, 320 buckets up to
distance 800) at B utterances of --seconds at 16 kHz.  One JSON line per batch size (appended to --out); every leg runs in one process,
alternated, two windows each of at least --window seconds (tools/hubert_bench.py's scheme: a pair is "separated" only where the faster
side's slowest window lies below the slower side's fastest by more than the two window spreads added):

  (a) wavlm f32 / wavlm bf16x3 against hubert f32 / hubert bf16x3 (features.HuBERT with the shared parameters' values): what the bias and
      the gate cost, with the per-kernel rows of the library's event profile for the attention and the gate-forming LayerNorm
  (b) wavlm f32 against the same function from stock PyTorch-ROCm operators (``stock_forward``: hubert_bench's with the (heads, T, T)
      bias materialised and handed to F.scaled_dot_product_attention as its mask)
  (c) layer=9 (the reference's linear_inference.py reads hidden_states[9]) against layer=-1
  (d) WavLM(layer=9) -> LinearHead against WavLM(layer=9) alone: the head's share of linear_inference

Weights are the constructors' random ones (the time does not depend on the values).
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from articulatory_amd import _native  # noqa: E402
from articulatory_amd.features import HuBERT, LinearHead, WavLM  # noqa: E402
from tools.hubert_bench import SR, alternated_legs, faster  # noqa: E402


def stock_forward(m, wav, layer=-1):
    """WavLM.forward(wav, layer=layer) for a batch of equal lengths, from stock operators on the module's own parameters."""
    c = m.config
    eps, heads = c["layer_norm_eps"], c["num_attention_heads"]
    x = (wav - wav.mean(-1, keepdim=True)) / torch.sqrt(wav.var(-1, unbiased=False, keepdim=True) + m.norm_eps)
    x = x[:, None]
    for lay, s in zip(m.feature_extractor.conv_layers, _native.HUBERT_CONV_STRIDE):
        x = F.conv1d(x, lay.conv.weight, lay.conv.bias, stride=s)
        x = F.gelu(F.layer_norm(x.transpose(1, 2), x.shape[1:2], lay.layer_norm.weight, lay.layer_norm.bias, 1e-5)).transpose(1, 2)
    x = x.transpose(1, 2)
    fp = m.feature_projection
    x = F.linear(F.layer_norm(x, x.shape[-1:], fp.layer_norm.weight, fp.layer_norm.bias, eps), fp.projection.weight, fp.projection.bias)
    pc = m.encoder.pos_conv_embed.conv
    g, v = pc.parametrizations.weight.original0, pc.parametrizations.weight.original1
    w = g * v / v.pow(2).sum((0, 1), keepdim=True).sqrt()
    x = x + F.gelu(F.conv1d(x.transpose(1, 2), w, pc.bias, padding=64, groups=16)[:, :, :-1]).transpose(1, 2)
    B, T, H = x.shape
    d = H // heads
    md = c["max_bucket_distance"]
    table = _native.wavlm_bucket_of_distance(c["num_buckets"], md).to(x.device).long()
    pos = torch.arange(T, device=x.device)
    bucket = table[(pos[None, :] - pos[:, None]).clamp(-md, md) + md]
    bias = m.encoder.layers[0].attention.rel_attn_embed(bucket).permute(2, 0, 1)  # (heads, T, T)
    layers = m.encoder.layers if layer < 0 else m.encoder.layers[:layer]
    for lay in layers:
        a = lay.attention
        n = F.layer_norm(x, (H,), lay.layer_norm.weight, lay.layer_norm.bias, eps)
        p = a.gru_rel_pos_linear(n.view(B, T, heads, d)).view(B, T, heads, 2, 4).sum(-1).sigmoid()
        gate = (p[..., 0] * (p[..., 1] * a.gru_rel_pos_const.view(1, 1, heads) - 1.0) + 2.0).transpose(1, 2)  # (B, heads, T)
        q, k, v = (F.linear(n, w_.weight, w_.bias).view(B, T, heads, d).transpose(1, 2) for w_ in (a.q_proj, a.k_proj, a.v_proj))
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=gate[..., None] * bias).transpose(1, 2).reshape(B, T, H)
        x = x + F.linear(o, a.out_proj.weight, a.out_proj.bias)
        n = F.layer_norm(x, (H,), lay.final_layer_norm.weight, lay.final_layer_norm.bias, eps)
        ff = lay.feed_forward
        x = x + F.linear(F.gelu(F.linear(n, ff.intermediate_dense.weight, ff.intermediate_dense.bias)), ff.output_dense.weight, ff.output_dense.bias)
    if layer < 0:
        x = F.layer_norm(x, (H,), m.encoder.layer_norm.weight, m.encoder.layer_norm.bias, eps)
    return x.transpose(1, 2)


def kernel_rows(m, fn, keys=("hubert_attn", "hubert_ln_kernel<gate", "hubert_ln_kernel")):
    """{profile row name: ms} of one call, for the rows whose name starts with one of ``keys`` (the LayerNorm rows without GELU: HuBERT's
    two per layer against WavLM's one plain and one gate-forming)."""
    lib, eng = m._lib, m.engine()
    lib.hificar_profile_begin(eng)
    fn()
    return {r["name"]: round(r["total_ms"], 3) for r in _native.profile_rows(lib, eng, 1024)[0]
            if r["name"].startswith(keys) and "gelu" not in r["name"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 8, 1])
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--limit", type=float, default=30.0, help="seconds a single call may take")
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--layer", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wavlm_bench: no GPU visible; a device time is measured on the device or not at all")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    models = {}
    for prec in ("f32", "bf16x3"):
        models[f"wavlm {prec}"] = WavLM(dict(num_hidden_layers=a.layers), precision=prec)
        models[f"hubert {prec}"] = HuBERT(dict(num_hidden_layers=a.layers), precision=prec)
    sd = models["wavlm f32"].state_dict()
    models["wavlm bf16x3"].load_state_dict(sd)
    for prec in ("f32", "bf16x3"):
        models[f"hubert {prec}"].load_state_dict({k: v for k, v in sd.items() if "gru_rel_pos" not in k and "rel_attn_embed" not in k})
    models = {k: m.cuda() for k, m in models.items()}
    wl = models["wavlm f32"]
    rng = np.random.default_rng(7)
    head = LinearHead(rng.standard_normal((12, 1024)) / 32.0, rng.standard_normal(12)).cuda()
    L = int(a.seconds * SR)
    lines = []
    with torch.no_grad():
        for B in a.batches:
            wav = 0.1 * torch.randn((B, L), generator=torch.Generator().manual_seed(B)).cuda()
            ref = stock_forward(wl, wav)
            err = {k: float((m(wav)[0] - ref).abs().max() / ref.abs().max()) for k, m in models.items() if k.startswith("wavlm")}
            ref9 = stock_forward(wl, wav, a.layer)
            err[f"wavlm f32 layer={a.layer}"] = float((wl(wav, layer=a.layer)[0] - ref9).abs().max() / ref9.abs().max())
            del ref, ref9
            names = list(models) + [f"wavlm f32 layer={a.layer}", f"wavlm f32 layer={a.layer} + head", "stock"]
            fns = [(lambda mm=m: mm(wav)) for m in models.values()]
            fns += [lambda: wl(wav, layer=a.layer), lambda: head(*wl(wav, layer=a.layer)), lambda: stock_forward(wl, wav)]
            ms = dict(zip(names, alternated_legs(fns, a.window, a.limit)))
            pairs = [("hubert f32", "wavlm f32"), ("hubert bf16x3", "wavlm bf16x3"), ("wavlm bf16x3", "wavlm f32"), ("wavlm f32", "stock"),
                     ("stock", "wavlm f32"), ("wavlm bf16x3", "stock"), (f"wavlm f32 layer={a.layer}", "wavlm f32"),
                     (f"wavlm f32 layer={a.layer}", f"wavlm f32 layer={a.layer} + head")]
            res = {"B": B, "samples": L, "layers": a.layers, "ms": ms,
                   "spread": {k: round(abs(w[0] - w[1]) / min(w), 4) for k, w in ms.items()},
                   "faster": {f"{x} < {y}": faster(ms[x], ms[y]) for x, y in pairs},
                   "ratio": {f"{y} / {x}": round(min(ms[y]) / max(ms[x]), 3) for x, y in pairs},
                   "rel_err_vs_stock": err, "workspace_mb": {k: round(m.workspace_bytes(B, L) / 1e6, 1) for k, m in models.items()},
                   "kernels_ms": {k: kernel_rows(m, lambda mm=m: mm(wav)) for k, m in models.items()}}
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
            del wav
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
