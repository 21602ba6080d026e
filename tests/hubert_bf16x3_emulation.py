"""What ``HuBERT(precision="bf16x3" | "bf16x3a")`` may cost in accuracy, predicted on the CPU: the float64 restatement tests/hubert_oracle.py
with every GEMM the conv engine runs — extractor layers 1 - 6, the projection, q | k | v, out_proj, intermediate_dense, output_dense —
computed as three split products summed in float64,

    x w  ~  hi(x) hi(w) + hi(x) lo(w) + lo(x) hi(w),      hi(a) = bf16(a), lo(a) = bf16(a - hi(a)),  a rounded to fp32 first,

which is the engine's split (round to nearest even, the subtraction exact in fp32).  With ``attn16=True`` Q K^T and P V are computed the
same way; P = exp(s - max) is split before the division by the row sum, which is taken from the unsplit exponentials.  Everything else
is float64, so the figures isolate what the dropped lo lo term and the operands' 16-bit tails cost; the device adds fp32 accumulation on top
(about 2e-6 of max|y| in exact fp32, tests/test_gpu_hubert.py).  The emulation predicts only: the device is compared against the float64
oracle (tests/test_gpu_hubert_bf16x3.py), at 2e-4 of max|y| per tensor, the project's bf16x3 bar.

``python tests/hubert_bf16x3_emulation.py`` prints the table of DESIGN.md §3.12.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hubert_oracle as O  # noqa: E402

SEED = 4242  # tests/test_hubert_host.py's
BAR = 1e-4   # every case below stays under it, so the device bar is the project's 2e-4


def bf16(x):
    """float32 array -> the nearest bf16 (ties to even), as float32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def split(x):
    """(hi, lo) of x rounded to fp32, as float64 arrays."""
    x32 = np.asarray(x, dtype=np.float64).astype(np.float32)
    hi = bf16(x32)
    lo = bf16(x32 - hi)
    return hi.astype(np.float64), lo.astype(np.float64)


def mm3(a, b):
    """a @ b with both operands split: hi hi + hi lo + lo hi, summed in float64."""
    ah, al = split(a)
    bh, bl = split(b)
    return ah @ bh + ah @ bl + al @ bh


def conv1d3(x, w, b, stride):
    """hubert_oracle.conv1d with every tap's product split."""
    k = w.shape[2]
    n = (x.shape[0] - k) // stride + 1
    y = np.zeros((n, w.shape[0]))
    for j in range(k):
        y += mm3(x[j:j + stride * (n - 1) + 1:stride], w[:, :, j].T)
    return y if b is None else y + b


def forward(sd, config, wav, attn16=False, do_normalize=True, norm_eps=O.NORM_EPS):
    """hubert_oracle.forward with the GEMMs of the bf16x3 forward (attn16: and the attention's products, bf16x3a) emulated."""
    f = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    eps = float(config.get("layer_norm_eps", 1e-5))
    heads = config["num_attention_heads"]
    x = np.asarray(wav, dtype=np.float64)
    if do_normalize:
        x = O.normalize(x, norm_eps)
    out = {}
    x = x[:, None]
    for i, (k, s) in enumerate(zip(O.KERNELS, O.STRIDES)):
        b = f"feature_extractor.conv_layers.{i}."
        conv = O.conv1d if i == 0 else conv1d3  # (layer 0: ten fp32 FMAs in a kernel of its own)
        x = conv(x, f[b + "conv.weight"], f.get(b + "conv.bias"), s)
        x = O.gelu(O.layer_norm(x, f[b + "layer_norm.weight"], f[b + "layer_norm.bias"], 1e-5))
        if i == 0:
            out["extractor.0"] = x
    out["extract_features"] = x
    x = O.layer_norm(x, f["feature_projection.layer_norm.weight"], f["feature_projection.layer_norm.bias"], eps)
    x = mm3(x, f["feature_projection.projection.weight"].T) + f["feature_projection.projection.bias"]
    out["feature_projection"] = x
    pos = O.pos_conv(x, O.pos_conv_weight(sd), f["encoder.pos_conv_embed.conv.bias"], config.get("num_conv_pos_embedding_groups", 16))
    out["pos_conv"] = pos
    x = x + pos
    hidden = []
    T, H = x.shape
    d = H // heads
    for l in range(config["num_hidden_layers"]):
        hidden.append(x)
        b = f"encoder.layers.{l}."
        n = O.layer_norm(x, f[b + "layer_norm.weight"], f[b + "layer_norm.bias"], eps)
        q, k, v = (mm3(n, f[b + f"attention.{w}_proj.weight"].T) + f[b + f"attention.{w}_proj.bias"] for w in "qkv")
        q, k, v = (t.reshape(T, heads, d).transpose(1, 0, 2) for t in (q, k, v))
        if attn16:
            s = np.stack([mm3(q[h], k[h].T) for h in range(heads)]) * d ** -0.5
            p = np.exp(s - s.max(-1, keepdims=True)).astype(np.float32).astype(np.float64)  # (the device's exponentials are fp32)
            a = np.stack([mm3(p[h], v[h]) for h in range(heads)]) / p.sum(-1, keepdims=True)
        else:
            s = q @ k.transpose(0, 2, 1) * d ** -0.5
            s = np.exp(s - s.max(-1, keepdims=True))
            a = (s / s.sum(-1, keepdims=True)) @ v
        a = a.transpose(1, 0, 2).reshape(T, H)
        x = x + mm3(a, f[b + "attention.out_proj.weight"].T) + f[b + "attention.out_proj.bias"]
        n = O.layer_norm(x, f[b + "final_layer_norm.weight"], f[b + "final_layer_norm.bias"], eps)
        hmid = O.gelu(mm3(n, f[b + "feed_forward.intermediate_dense.weight"].T) + f[b + "feed_forward.intermediate_dense.bias"])
        x = x + mm3(hmid, f[b + "feed_forward.output_dense.weight"].T) + f[b + "feed_forward.output_dense.bias"]
    x = O.layer_norm(x, f["encoder.layer_norm.weight"], f["encoder.layer_norm.bias"], eps)
    hidden.append(x)
    out["hidden_states"] = hidden
    out["last_hidden_state"] = x
    return out


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def tiny():
    return dict(conv_dim=[64] * 7, conv_kernel=list(O.KERNELS), conv_stride=list(O.STRIDES), hidden_size=128, num_attention_heads=2, intermediate_size=256,
                num_hidden_layers=2, conv_bias=True, feat_extract_norm="layer", do_stable_layer_norm=True, feat_proj_layer_norm=True,
                layer_norm_eps=1e-5, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, hidden_act="gelu",
                feat_extract_activation="gelu", mask_time_prob=0.05, mask_feature_prob=0.0)


def samples(frames):
    return 400 + 320 * (frames - 1)


def cases():
    """name -> (config, gain, wav seed, samples): the inputs of tests/test_gpu_hubert.py's cases, and the same at gain 2."""
    t = tiny()
    out = {f"tiny, {n} frames": (t, 1.0, SEED + samples(n), samples(n)) for n in (1, 65, 149)}
    out["tiny, 719 samples"] = (t, 1.0, SEED + 719, 719)
    out["tiny width, 24 layers, 3 s"] = (dict(t, num_hidden_layers=24), 1.0, SEED + 2, 48000)
    out["tiny, 65 frames, gain 2 weights"] = (t, 2.0, SEED + samples(65), samples(65))
    out["conv 512 / hidden 1024 / 16 heads / FFN 4096, 4 layers, 1 s"] = (
        dict(t, conv_dim=[512] * 7, hidden_size=1024, num_attention_heads=16, intermediate_size=4096, num_hidden_layers=4), 1.0, SEED + 1, 16000)
    return out


def max_logit(sd, config, ref):
    """max |logit| over layers and heads of the float64 forward (how flat the softmax is)."""
    H, heads, worst = config["hidden_size"], config["num_attention_heads"], 0.0
    d = H // heads
    eps = float(config.get("layer_norm_eps", 1e-5))
    for l in range(config["num_hidden_layers"]):
        b = f"encoder.layers.{l}."
        n = O.layer_norm(ref["hidden_states"][l], np.asarray(sd[b + "layer_norm.weight"], np.float64), np.asarray(sd[b + "layer_norm.bias"], np.float64), eps)
        q, k = (n @ np.asarray(sd[b + f"attention.{w}_proj.weight"], np.float64).T + np.asarray(sd[b + f"attention.{w}_proj.bias"], np.float64) for w in "qk")
        T = n.shape[0]
        q, k = (t.reshape(T, heads, d).transpose(1, 0, 2) for t in (q, k))
        worst = max(worst, float(np.abs(q @ k.transpose(0, 2, 1)).max() * d ** -0.5))
    return worst


def measure(name):
    """{"bf16x3", "bf16x3a": max |delta| / max |y| over the last hidden state and every hidden_states[k]; "extract_features"; "max_logit"}."""
    from articulatory_amd.utils.synth import synth_hubert_state_dict

    config, gain, seed, L = cases()[name]
    sd = synth_hubert_state_dict(config, seed=SEED, gain=gain)
    wav = O.synth_wav(seed, L)
    ref = O.forward(sd, config, wav)
    res = {"max_logit": max_logit(sd, config, ref)}
    for tag, a16 in (("bf16x3", False), ("bf16x3a", True)):
        got = forward(sd, config, wav, attn16=a16)
        res[tag] = max(rel(g, r) for g, r in zip(got["hidden_states"], ref["hidden_states"]))
        res["extract_features"] = rel(got["extract_features"], ref["extract_features"])
    return res


if __name__ == "__main__":
    print("| case | bf16x3 | bf16x3a | extract_features | max logit |")
    print("|---|---|---|---|---|")
    for name in cases():
        r = measure(name)
        print(f"| {name} | {r['bf16x3']:.1e} | {r['bf16x3a']:.1e} | {r['extract_features']:.1e} | {r['max_logit']:.1f} |", flush=True)
