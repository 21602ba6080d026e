"""What ``WavLM(precision="bf16x3")`` may cost in accuracy, predicted on the CPU: tests/hubert_bf16x3_emulation.py's emulation — every GEMM
of the conv engine as three split products summed in float64 — with WavLM's gated relative position bias added to the scores as the device
adds it: in fp32 arithmetic there, float64 here; the gates come from the unsplit LayerNorm output (the device takes them from the LayerNorm
kernel's registers, not from hi + lo).  The bias makes the logits larger (the synthetic table is N(0, 1), the gates 1.4 .. 2.1), so the
softmax is less flat than HuBERT's on the same weights and an error of q | k | v weighs more: hence a figure of its own.

The bar of tests/test_gpu_wavlm.py's bf16x3 cases follows from ``worst()``: HuBERT's 2e-4 of max|y| if the worst tensor stays within a
quarter of it (5e-5), else four times the worst.  ``python tests/wavlm_bf16x3_emulation.py`` prints the table of DESIGN.md §3.13.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hubert_bf16x3_emulation as E  # noqa: E402
import hubert_oracle as O  # noqa: E402
import wavlm_oracle as W  # noqa: E402

SEED = E.SEED
FRAMES = (1, 2, 30, 63, 64, 65, 128, 129, 149)  # tests/test_gpu_wavlm.py's
HUBERT_BAR = 2e-4


def tiny():
    return dict(E.tiny(), num_buckets=32, max_bucket_distance=24)


def forward(sd, config, wav):
    """wavlm_oracle.forward with the GEMMs of the bf16x3 forward emulated."""
    f = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    eps = float(config.get("layer_norm_eps", 1e-5))
    heads = config["num_attention_heads"]
    x = O.normalize(np.asarray(wav, dtype=np.float64))[:, None]
    for i, (k, s) in enumerate(zip(O.KERNELS, O.STRIDES)):
        b = f"feature_extractor.conv_layers.{i}."
        conv = O.conv1d if i == 0 else E.conv1d3
        x = O.gelu(O.layer_norm(conv(x, f[b + "conv.weight"], f.get(b + "conv.bias"), s), f[b + "layer_norm.weight"], f[b + "layer_norm.bias"], 1e-5))
    x = O.layer_norm(x, f["feature_projection.layer_norm.weight"], f["feature_projection.layer_norm.bias"], eps)
    x = E.mm3(x, f["feature_projection.projection.weight"].T) + f["feature_projection.projection.bias"]
    x = x + O.pos_conv(x, O.pos_conv_weight(sd), f["encoder.pos_conv_embed.conv.bias"], config.get("num_conv_pos_embedding_groups", 16))
    T, H = x.shape
    d = H // heads
    bias = W.position_bias(sd, config, T)
    hidden, gate_list = [], []
    for l in range(config["num_hidden_layers"]):
        hidden.append(x)
        b = f"encoder.layers.{l}."
        n = O.layer_norm(x, f[b + "layer_norm.weight"], f[b + "layer_norm.bias"], eps)
        g = W.gates(n, f[b + "attention.gru_rel_pos_linear.weight"], f[b + "attention.gru_rel_pos_linear.bias"], f[b + "attention.gru_rel_pos_const"], heads)
        gate_list.append(g)
        q, k, v = (E.mm3(n, f[b + f"attention.{w}_proj.weight"].T) + f[b + f"attention.{w}_proj.bias"] for w in "qkv")
        q, k, v = (t.reshape(T, heads, d).transpose(1, 0, 2) for t in (q, k, v))
        s = q @ k.transpose(0, 2, 1) * d ** -0.5 + g[:, :, None] * bias
        s = np.exp(s - s.max(-1, keepdims=True))
        a = ((s / s.sum(-1, keepdims=True)) @ v).transpose(1, 0, 2).reshape(T, H)
        x = x + E.mm3(a, f[b + "attention.out_proj.weight"].T) + f[b + "attention.out_proj.bias"]
        n = O.layer_norm(x, f[b + "final_layer_norm.weight"], f[b + "final_layer_norm.bias"], eps)
        hmid = O.gelu(E.mm3(n, f[b + "feed_forward.intermediate_dense.weight"].T) + f[b + "feed_forward.intermediate_dense.bias"])
        x = x + E.mm3(hmid, f[b + "feed_forward.output_dense.weight"].T) + f[b + "feed_forward.output_dense.bias"]
    x = O.layer_norm(x, f["encoder.layer_norm.weight"], f["encoder.layer_norm.bias"], eps)
    hidden.append(x)
    return {"hidden_states": hidden, "last_hidden_state": x, "gates": gate_list}


def measure(frames):
    """max |delta| / max |y| over the last hidden state and every hidden_states[k] of the tiny model at ``frames`` frames."""
    from articulatory_amd.utils.synth import synth_wavlm_state_dict

    config = tiny()
    sd = synth_wavlm_state_dict(config, seed=SEED)
    L = E.samples(frames)
    wav = O.synth_wav(SEED + L, L)
    ref, got = W.forward(sd, config, wav), forward(sd, config, wav)
    return max(E.rel(g, r) for g, r in zip(got["hidden_states"], ref["hidden_states"]))


def worst():
    return max(measure(n) for n in FRAMES)


def bar():
    """The device bar of the bf16x3 cases, by the rule above."""
    w = worst()
    return HUBERT_BAR if w <= HUBERT_BAR / 4 else 4 * w


if __name__ == "__main__":
    print("| frames | bf16x3, worst tensor |")
    print("|---|---|")
    for n in FRAMES:
        print(f"| {n} | {measure(n):.1e} |", flush=True)
    print("bar", bar())
