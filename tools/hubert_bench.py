#!/usr/bin/env python3
"""Device time of the native HuBERT encoder (articulatory_amd.features.HuBERT, the large model: 24 x 1024, conv 512) at B utterances of
--seconds at 16 kHz, against the same function written from stock PyTorch-ROCm operators (``stock_forward`` below: F.conv1d, F.layer_norm,
F.gelu, F.linear, F.scaled_dot_product_attention in fp32).

One JSON line per batch size (appended to --out):

  native_ms / stock_ms   device milliseconds per call, two windows each of at least --window seconds, alternated native / stock / native /
                         stock in one process: the two windows of a side run on unchanged code, so their difference is the spread a reader
                         should hold the difference between the sides against ("separated" = the sides' windows do not overlap)
  kernels_ms             per-kernel-group device time of one native call from the library's event profile; posconv_share and gelu_share are
                         the positional conv's and the GELU pass's parts of the sum
  tflops                 achieved TFLOP/s of the native call, from the FLOP count of the shapes (2 x MACs of every conv, GEMM and the
                         attention's two products), beside the 157.3 TFLOP/s fp32-MFMA peak
  ema                    HuBERT -> BiGRU.forward_lowrate(interp_factor=4) against the forward_lowrate alone on states already there: the
                         encoder's share of speech -> EMA

--precision bf16x3 | bf16x3a adds that arithmetic's leg to the alternation: native f32 / native P / stock (bf16x3a: native f32 / native
bf16x3 / native bf16x3a / stock — its yardstick is the bf16x3 leg of the same run), two windows per leg, on a copy of the same model.  The
line gains "precision" and "legs": per leg its windows, spread, per-kernel groups, workspace and error against stock, and per pair
(leg against its yardstick) "faster": true only where the leg's slowest window lies below the yardstick's fastest by more than the two
window spreads added.  Without the flag the tool does what it did.

Weights are the constructors' random ones (the time does not depend on the values).
"""

import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from articulatory_amd import _native  # noqa: E402
from articulatory_amd.features import HuBERT  # noqa: E402
from articulatory_amd.models import BiGRU  # noqa: E402
from articulatory_amd.utils.synth import synth_bigru_state_dict  # noqa: E402
from tools.features_bench import alternated, window  # noqa: E402

SR = 16000
PEAK_TFLOPS = 157.3
BIGRU = dict(in_channels=1024, hidden_size=256, out_channels=12, use_tanh=True)


def stock_forward(m, wav):
    """HuBERT.forward(wav) for a batch of equal lengths, from stock operators on the module's own parameters."""
    c = m.config
    eps, heads = c["layer_norm_eps"], c["num_attention_heads"]
    x = (wav - wav.mean(-1, keepdim=True)) / torch.sqrt(wav.var(-1, unbiased=False, keepdim=True) + m.norm_eps)
    x = x[:, None]
    for layer, s in zip(m.feature_extractor.conv_layers, _native.HUBERT_CONV_STRIDE):
        x = F.conv1d(x, layer.conv.weight, layer.conv.bias, stride=s)
        x = F.gelu(F.layer_norm(x.transpose(1, 2), x.shape[1:2], layer.layer_norm.weight, layer.layer_norm.bias, 1e-5)).transpose(1, 2)
    x = x.transpose(1, 2)
    fp = m.feature_projection
    x = F.linear(F.layer_norm(x, x.shape[-1:], fp.layer_norm.weight, fp.layer_norm.bias, eps), fp.projection.weight, fp.projection.bias)
    pc = m.encoder.pos_conv_embed.conv
    g, v = pc.parametrizations.weight.original0, pc.parametrizations.weight.original1
    w = g * v / v.pow(2).sum((0, 1), keepdim=True).sqrt()
    pos = F.conv1d(x.transpose(1, 2), w, pc.bias, padding=64, groups=16)[:, :, :-1]
    x = x + F.gelu(pos).transpose(1, 2)
    B, T, H = x.shape
    for layer in m.encoder.layers:
        a = layer.attention
        n = F.layer_norm(x, (H,), layer.layer_norm.weight, layer.layer_norm.bias, eps)
        q, k, v = (F.linear(n, p.weight, p.bias).view(B, T, heads, H // heads).transpose(1, 2) for p in (a.q_proj, a.k_proj, a.v_proj))
        o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, H)
        x = x + F.linear(o, a.out_proj.weight, a.out_proj.bias)
        n = F.layer_norm(x, (H,), layer.final_layer_norm.weight, layer.final_layer_norm.bias, eps)
        ff = layer.feed_forward
        x = x + F.linear(F.gelu(F.linear(n, ff.intermediate_dense.weight, ff.intermediate_dense.bias)), ff.output_dense.weight, ff.output_dense.bias)
    x = F.layer_norm(x, (H,), m.encoder.layer_norm.weight, m.encoder.layer_norm.bias, eps)
    return x.transpose(1, 2)


def flop_count(c, B, L):
    """FLOP of one forward from the shapes: 2 x MACs of the convs, the GEMMs and the attention's Q K^T and P V."""
    C, H, I, N = c["conv_dim"][0], c["hidden_size"], c["intermediate_size"], c["num_hidden_layers"]
    t, macs = L, 0.0
    for i, (k, s) in enumerate(zip(_native.HUBERT_CONV_KERNEL, _native.HUBERT_CONV_STRIDE)):
        t = (t - k) // s + 1
        macs += t * C * (1 if i == 0 else C) * k
    macs += t * (C * H + H * (H // 16) * 128)
    macs += N * t * (4 * H * H + 2 * H * I + 2 * t * H)
    return 2.0 * macs * B, t


def group(name):
    for key, label in (("hubert_conv0", "extractor layer 0"), ("#window", "extractor convs 1-6"), ("hubert_ln_kernel<gelu", "extractor LayerNorm + GELU"),
                       ("hubert_posconv", "positional conv"), ("hubert_attn", "attention"), ("hubert_gelu", "GELU pass"), ("hubert_ln", "LayerNorm"),
                       ("conv_", "GEMMs")):
        if key in name:
            return label
    return "other"


def kernel_groups(m, fn):
    lib, eng = m._lib, m.engine()
    lib.hificar_profile_begin(eng)  # with HIFICAR_PROFILE_DETAIL=1 the conv rows carry their layer's name
    fn()
    out = {}
    for r in _native.profile_rows(lib, eng, 1024)[0]:
        out[group(r["name"])] = out.get(group(r["name"]), 0.0) + r["total_ms"]
    return {k: round(v, 3) for k, v in sorted(out.items(), key=lambda kv: -kv[1])}


def alternated_legs(fns, seconds, limit):
    """features_bench.alternated for any number of legs: leg 0, 1, .., 0, 1, ..; two windows each."""
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    first = [window(fn, seconds, limit) for fn in fns]
    second = [window(fn, seconds, limit) for fn in fns]
    return [[round(a, 4), round(b, 4)] for a, b in zip(first, second)]


def faster(leg, yard):
    """The leg's slowest window lies below the yardstick's fastest by more than the two window spreads added."""
    return bool(min(yard) - max(leg) > abs(leg[0] - leg[1]) + abs(yard[0] - yard[1]))


def precision_legs(m, bigru, wav, ref, frames, precision, a):
    """The "legs" entry of a line: native f32, (bf16x3,) `precision` and stock alternated in one process."""
    names = ["f32"] + (["bf16x3"] if precision == "bf16x3a" else []) + [precision]
    models = {"f32": m}
    for n in names[1:]:
        models[n] = copy.deepcopy(m)
        models[n].set_precision(n)
    B, L = wav.shape
    legs = {}
    for n in names:
        got = models[n](wav)[0]
        legs[n] = {"rel_err_vs_stock": float((got - ref).abs().max() / ref.abs().max()), "workspace_mb": round(models[n].workspace_bytes(B, L) / 1e6, 1)}
        del got
    ms = alternated_legs([(lambda mm=models[n]: mm(wav)) for n in names] + [lambda: stock_forward(m, wav)], a.window, a.limit)
    for n, w in zip(names + ["stock"], ms):
        legs.setdefault(n, {})["ms"] = w
        legs[n]["spread"] = round(abs(w[0] - w[1]) / min(w), 4)
    for n in names:
        legs[n]["kernels_ms"] = kernel_groups(models[n], lambda mm=models[n]: mm(wav))
    pairs = [(names[i], names[i - 1]) for i in range(1, len(names))] + [(n, "stock") for n in names]
    out = {"legs": legs, "faster": {f"{x} < {y}": faster(legs[x]["ms"], legs[y]["ms"]) for x, y in pairs},
           "ratio": {f"{y} / {x}": round(min(legs[y]["ms"]) / max(legs[x]["ms"]), 3) for x, y in pairs}}
    mp = models[precision]
    e_ms, b_ms = alternated(lambda: bigru.forward_lowrate(mp(wav)[0], lengths=frames, interp_factor=4),
                            lambda: bigru.forward_lowrate(ref, lengths=frames, interp_factor=4), a.window, a.limit)
    out["ema"] = {"speech_to_ema_ms": e_ms, "forward_lowrate_ms": b_ms, "encoder_share": round((min(e_ms) - max(b_ms)) / min(e_ms), 4)}
    for n in names[1:]:
        models[n]._invalidate()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--limit", type=float, default=30.0, help="seconds a single call may take")
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--precision", default=None, choices=("bf16x3", "bf16x3a"), help="add this arithmetic's leg(s) to the alternation")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hubert_bench: no GPU visible; a device time is measured on the device or not at all")
    os.environ.setdefault("HIFICAR_PROFILE_DETAIL", "1")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    m = HuBERT(dict(num_hidden_layers=a.layers)).cuda()
    bigru = BiGRU(**BIGRU)
    bigru.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth_bigru_state_dict(BIGRU, seed=5101).items()}, strict=True)
    bigru = bigru.eval().cuda()
    L = int(a.seconds * SR)
    lines = []
    with torch.no_grad():
        for B in a.batches:
            wav = 0.1 * torch.randn((B, L), generator=torch.Generator().manual_seed(B)).cuda()
            ref = stock_forward(m, wav)
            got, frames = m(wav)
            err = float((got - ref).abs().max() / ref.abs().max())
            n_ms, s_ms = alternated(lambda: m(wav), lambda: stock_forward(m, wav), a.window, a.limit)
            flop, T = flop_count(m.config, B, L)
            kern = kernel_groups(m, lambda: m(wav))
            total = sum(kern.values())
            e_ms, b_ms = alternated(lambda: bigru.forward_lowrate(m(wav)[0], lengths=frames, interp_factor=4),
                                    lambda: bigru.forward_lowrate(got, lengths=frames, interp_factor=4), a.window, a.limit)
            res = {"B": B, "samples": L, "frames": T, "layers": a.layers, "native_ms": n_ms, "stock_ms": s_ms,
                   "native_spread": round(abs(n_ms[0] - n_ms[1]) / min(n_ms), 4), "stock_spread": round(abs(s_ms[0] - s_ms[1]) / min(s_ms), 4),
                   "separated": max(n_ms) < min(s_ms) or max(s_ms) < min(n_ms), "stock_over_native": round(min(s_ms) / max(n_ms), 3),
                   "native_vs_stock_rel_err": err, "gflop": round(flop / 1e9, 1), "tflops": round(flop / (min(n_ms) * 1e9), 2),
                   "peak_tflops": PEAK_TFLOPS, "workspace_mb": round(m.workspace_bytes(B, L) / 1e6, 1), "kernels_ms": kern,
                   "posconv_share": round(kern.get("positional conv", 0.0) / total, 4), "gelu_share": round(kern.get("GELU pass", 0.0) / total, 4),
                   "ema": {"speech_to_ema_ms": e_ms, "forward_lowrate_ms": b_ms, "encoder_share": round((min(e_ms) - max(b_ms)) / min(e_ms), 4)}}
            if a.precision:
                res["precision"] = a.precision
                res["opt_in"] = precision_legs(m, bigru, wav, ref, frames, a.precision, a)
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
            del wav, ref, got
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
