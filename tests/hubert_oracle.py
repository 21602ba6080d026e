"""float64 numpy restatement of the HuBERT encoder, "large" family (layer-norm extractor, stable layer norm), one utterance at a time:
the yardstick of tests/test_gpu_hubert.py, pinned to the ``transformers`` library's ``HubertModel`` (run in float64) by
tests/golden/gold_hubert.npz at 1e-9 (tests/test_hubert_host.py).  ``sd``: a ``HubertModel``-layout state_dict of numpy arrays
(``articulatory_amd.utils.synth.synth_hubert_state_dict``); ``config``: a mapping with the keys of its ``config.json``.
"""

import math

import numpy as np

KERNELS = (10, 3, 3, 3, 3, 2, 2)
STRIDES = (5, 2, 2, 2, 2, 2, 2)
NORM_EPS = 1e-7  # Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm



def _erf(x):
    import torch  # (numpy has no erf; torch's float64 one agrees with math.erf to the last bit or two)

    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def frames(length):
    """50-Hz frames of ``length`` samples: the seven convs' output lengths composed; 0 under 400 samples."""
    return (int(length) - 400) // 320 + 1 if length >= 400 else 0


def gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def layer_norm(x, w, b, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def normalize(wav, eps=NORM_EPS):
    wav = np.asarray(wav, dtype=np.float64)
    return (wav - wav.mean()) / np.sqrt(wav.var() + eps)


def conv1d(x, w, b, stride):
    """x (T, Cin), w (Cout, Cin, k) -> (T_out, Cout), no padding."""
    k = w.shape[2]
    n = (x.shape[0] - k) // stride + 1
    y = np.zeros((n, w.shape[0]))
    for j in range(k):
        y += x[j:j + stride * (n - 1) + 1:stride] @ w[:, :, j].T
    return y if b is None else y + b


def pos_conv_weight(sd):
    p = "encoder.pos_conv_embed.conv."
    g = sd.get(p + "parametrizations.weight.original0", sd.get(p + "weight_g"))
    v = sd.get(p + "parametrizations.weight.original1", sd.get(p + "weight_v"))
    g, v = np.asarray(g, np.float64), np.asarray(v, np.float64)
    return g * v / np.sqrt((v ** 2).sum(axis=(0, 1), keepdims=True))  # weight_norm over dim 2


def pos_conv(x, w, b, groups):
    """Conv1d(H, H, K, padding K // 2, groups) of x (T, H) without its last frame (K even), + bias, GELU."""
    T, H = x.shape
    K, G = w.shape[2], H // groups
    xp = np.zeros((T + K, H))
    xp[K // 2:K // 2 + T] = x
    wg = w.reshape(groups, G, G, K)  # [group][out][in][tap]
    y = np.zeros((T, groups, G))
    for k in range(K):
        y += np.einsum("tgc,goc->tgo", xp[k:k + T].reshape(T, groups, G), wg[:, :, :, k])
    return gelu(y.reshape(T, H) + b)


def forward(sd, config, wav, do_normalize=True, norm_eps=NORM_EPS):
    """One utterance (1-D samples) -> dict: "extractor.0" (T0, C), "extract_features" (T, C), "feature_projection", "pos_conv" (T, H),
    "hidden_states" (the list ``output_hidden_states=True`` returns: N + 1 arrays (T, H)) and "last_hidden_state" (its last entry)."""
    f = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    eps = float(config.get("layer_norm_eps", 1e-5))
    heads = config["num_attention_heads"]
    x = np.asarray(wav, dtype=np.float64)
    if do_normalize:
        x = normalize(x, norm_eps)
    out = {}
    x = x[:, None]
    for i, (k, s) in enumerate(zip(KERNELS, STRIDES)):
        b = f"feature_extractor.conv_layers.{i}."
        x = conv1d(x, f[b + "conv.weight"], f.get(b + "conv.bias"), s)
        x = gelu(layer_norm(x, f[b + "layer_norm.weight"], f[b + "layer_norm.bias"], 1e-5))  # (torch.nn.LayerNorm's default eps)
        if i == 0:
            out["extractor.0"] = x
    out["extract_features"] = x
    x = layer_norm(x, f["feature_projection.layer_norm.weight"], f["feature_projection.layer_norm.bias"], eps)
    x = x @ f["feature_projection.projection.weight"].T + f["feature_projection.projection.bias"]
    out["feature_projection"] = x
    pos = pos_conv(x, pos_conv_weight(sd), f["encoder.pos_conv_embed.conv.bias"], config.get("num_conv_pos_embedding_groups", 16))
    out["pos_conv"] = pos
    x = x + pos
    hidden = []
    T, H = x.shape
    d = H // heads
    for l in range(config["num_hidden_layers"]):
        hidden.append(x)
        b = f"encoder.layers.{l}."
        n = layer_norm(x, f[b + "layer_norm.weight"], f[b + "layer_norm.bias"], eps)
        q, k, v = (n @ f[b + f"attention.{w}_proj.weight"].T + f[b + f"attention.{w}_proj.bias"] for w in "qkv")
        q, k, v = (t.reshape(T, heads, d).transpose(1, 0, 2) for t in (q, k, v))
        s = q @ k.transpose(0, 2, 1) * d ** -0.5
        s = np.exp(s - s.max(-1, keepdims=True))
        a = (s / s.sum(-1, keepdims=True)) @ v
        a = a.transpose(1, 0, 2).reshape(T, H)
        x = x + a @ f[b + "attention.out_proj.weight"].T + f[b + "attention.out_proj.bias"]
        n = layer_norm(x, f[b + "final_layer_norm.weight"], f[b + "final_layer_norm.bias"], eps)
        hmid = gelu(n @ f[b + "feed_forward.intermediate_dense.weight"].T + f[b + "feed_forward.intermediate_dense.bias"])
        x = x + hmid @ f[b + "feed_forward.output_dense.weight"].T + f[b + "feed_forward.output_dense.bias"]
    x = layer_norm(x, f["encoder.layer_norm.weight"], f["encoder.layer_norm.bias"], eps)
    hidden.append(x)
    out["hidden_states"] = hidden
    out["last_hidden_state"] = x
    return out


def synth_wav(seed, length, amplitude=0.1, offset=0.0):
    """Pseudo-speech of ``length`` samples: a few harmonics and noise from the name-keyed generator (float32, as a wav file holds it)."""
    from articulatory_amd.utils.synth import uniform

    t = np.arange(length, dtype=np.float64) / 16000.0
    f0 = 95.0 + 3.0 * (seed % 17)
    amp = uniform(seed, "hubert.wav.amp", (6,), 0.2, 1.0).astype(np.float64)
    y = sum(amp[h] * np.sin(2 * np.pi * f0 * (h + 1) * t + 0.4 * h) for h in range(6)) / 6.0
    y = y + uniform(seed, f"hubert.wav.noise.{length}", (length,), -0.3, 0.3)
    return (amplitude * y + offset).astype(np.float32)
