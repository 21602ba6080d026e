"""float64 numpy restatement of the WavLM encoder, "large" family (HuBERT-large's layers with the gated relative position bias), one utterance
at a time: the yardstick of tests/test_gpu_wavlm.py, pinned to the ``transformers`` library's ``WavLMModel`` (run in float64) by
tests/golden/gold_wavlm.npz at 1e-10 (tests/test_wavlm_host.py).  Everything in front of the layers, the LayerNorms and the feed-forward are
tests/hubert_oracle.py's.  ``sd``: a ``WavLMModel``-layout state_dict of numpy arrays (``utils.synth.synth_wavlm_state_dict``).

``variant`` breaks one thing on purpose, for the test that shows the fixtures would notice: ``"no_bias"`` (bias zeroed), ``"negated"``
(k - q negated), ``"gate_one"`` (gate fixed to 1), ``"clamp_exact"`` (distance clamped at the last exact bucket instead of max_distance).
"""

import math

import numpy as np

try:
    import hubert_oracle as O
except ImportError:  # (imported as tests.wavlm_oracle, from outside pytest)
    from tests import hubert_oracle as O

NORM_EPS, frames, synth_wav = O.NORM_EPS, O.frames, O.synth_wav

VARIANTS = ("no_bias", "negated", "gate_one", "clamp_exact")


def bucket(d, num_buckets, max_distance):
    """The library's ``_relative_positions_bucket`` of an integer array of relative positions (key - query); the logarithm in float32 by
    torch, as there."""
    import torch

    d = torch.from_numpy(np.ascontiguousarray(d, dtype=np.int64))
    nb = num_buckets // 2
    me = nb // 2
    a = d.abs()
    large = torch.log(a.float() / me) / math.log(max_distance / me) * (nb - me)
    large = torch.clamp((me + large).to(torch.long), max=nb - 1)
    return ((d > 0).long() * nb + torch.where(a < me, a, large)).numpy()


def position_bias(sd, config, T, variant=None):
    """(heads, T, T): rel_attn_embed[bucket(k - q), h]."""
    nb, md = config.get("num_buckets", 320), config.get("max_bucket_distance", 800)
    d = np.arange(T)[None, :] - np.arange(T)[:, None]  # [q, k] = k - q
    if variant == "negated":
        d = -d
    if variant == "clamp_exact":
        d = np.clip(d, -(nb // 4), nb // 4)
    emb = np.asarray(sd["encoder.layers.0.attention.rel_attn_embed.weight"], dtype=np.float64)
    bias = emb[bucket(d, nb, md)].transpose(2, 0, 1)
    return np.zeros_like(bias) if variant == "no_bias" else bias


def gates(n, w, b, const, heads):
    """n (T, H): the layer's attention input; -> (heads, T)."""
    T, H = n.shape
    p = n.reshape(T, heads, H // heads) @ w.T + b  # (T, heads, 8)
    s = 1.0 / (1.0 + np.exp(-p.reshape(T, heads, 2, 4).sum(-1)))
    ga, gb = s[..., 0], s[..., 1]
    return (ga * (gb * const.reshape(1, heads) - 1.0) + 2.0).T


def forward(sd, config, wav, do_normalize=True, norm_eps=NORM_EPS, variant=None):
    """One utterance (1-D samples) -> dict: "extract_features", "feature_projection", "pos_conv", "hidden_states" (N + 1 arrays (T, H)),
    "last_hidden_state" and "gates" (N arrays (heads, T))."""
    assert variant is None or variant in VARIANTS
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
        x = O.conv1d(x, f[b + "conv.weight"], f.get(b + "conv.bias"), s)
        x = O.gelu(O.layer_norm(x, f[b + "layer_norm.weight"], f[b + "layer_norm.bias"], 1e-5))
    out["extract_features"] = x
    x = O.layer_norm(x, f["feature_projection.layer_norm.weight"], f["feature_projection.layer_norm.bias"], eps)
    x = x @ f["feature_projection.projection.weight"].T + f["feature_projection.projection.bias"]
    out["feature_projection"] = x
    pos = O.pos_conv(x, O.pos_conv_weight(sd), f["encoder.pos_conv_embed.conv.bias"], config.get("num_conv_pos_embedding_groups", 16))
    out["pos_conv"] = pos
    x = x + pos
    T, H = x.shape
    d = H // heads
    bias = position_bias(sd, config, T, variant)
    hidden, gate_list = [], []
    for l in range(config["num_hidden_layers"]):
        hidden.append(x)
        b = f"encoder.layers.{l}."
        n = O.layer_norm(x, f[b + "layer_norm.weight"], f[b + "layer_norm.bias"], eps)
        g = gates(n, f[b + "attention.gru_rel_pos_linear.weight"], f[b + "attention.gru_rel_pos_linear.bias"], f[b + "attention.gru_rel_pos_const"], heads)
        gate_list.append(g)
        if variant == "gate_one":
            g = np.ones_like(g)
        q, k, v = (n @ f[b + f"attention.{w}_proj.weight"].T + f[b + f"attention.{w}_proj.bias"] for w in "qkv")
        q, k, v = (t.reshape(T, heads, d).transpose(1, 0, 2) for t in (q, k, v))
        s = q @ k.transpose(0, 2, 1) * d ** -0.5 + g[:, :, None] * bias
        s = np.exp(s - s.max(-1, keepdims=True))
        a = (s / s.sum(-1, keepdims=True)) @ v
        a = a.transpose(1, 0, 2).reshape(T, H)
        x = x + a @ f[b + "attention.out_proj.weight"].T + f[b + "attention.out_proj.bias"]
        n = O.layer_norm(x, f[b + "final_layer_norm.weight"], f[b + "final_layer_norm.bias"], eps)
        hmid = O.gelu(n @ f[b + "feed_forward.intermediate_dense.weight"].T + f[b + "feed_forward.intermediate_dense.bias"])
        x = x + hmid @ f[b + "feed_forward.output_dense.weight"].T + f[b + "feed_forward.output_dense.bias"]
    x = O.layer_norm(x, f["encoder.layer_norm.weight"], f["encoder.layer_norm.bias"], eps)
    hidden.append(x)
    out["hidden_states"] = hidden
    out["last_hidden_state"] = x
    out["gates"] = gate_list
    return out
