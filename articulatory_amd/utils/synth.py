"""Deterministic synthetic checkpoints for the HiFi-GAN / HiFi-CAR generator.

Trained checkpoints of the reference are Google-Drive links (reference README.md:36)
and unreachable offline, so every parity test, golden fixture and benchmark in this
repo runs on *synthesised* weights.  The generator here is numpy-only and keyed by
tensor name, so that

  * the golden-vector script (oracle/make_golden.py, which imports the real reference),
  * the CPU oracle (oracle/hificar_oracle.py),
  * the HIP path (articulatory_amd.models.HiFiGANGenerator) and
  * bench.py

all regenerate bit-identical fp32 tensors from (seed, name, shape) without shipping
the 54 MB state_dict.  The tensors are produced in the reference's *checkpoint*
layout: ``*.weight_g`` / ``*.weight_v`` / ``*.bias`` for every Conv1d/ConvTranspose1d
(old-style ``torch.nn.utils.weight_norm``; reference articulatory/models/hifigan.py:268-278)
and plain ``weight`` / ``bias`` for the PastFCEncoder Linear layers
(reference articulatory/layers/pytorch_layers.py:438-449).
"""

from collections import OrderedDict

import numpy as np

_MASK = np.uint64(0xFFFFFFFFFFFFFFFF)


def _fnv1a64(name: str) -> int:
    h = 0xCBF29CE484222325
    for b in name.encode("utf-8"):
        h ^= b
        h = (h * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _splitmix64(x: np.ndarray) -> np.ndarray:
    """Vectorised splitmix64 finaliser on a uint64 array (wrap-around arithmetic)."""
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15)) & _MASK
        z = x
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _MASK
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _MASK
        z = z ^ (z >> np.uint64(31))
    return z


def uniform01(seed: int, name: str, n: int) -> np.ndarray:
    """n float64 samples in [0, 1), a pure function of (seed, name, index)."""
    base = (_fnv1a64(name) ^ (int(seed) * 0xD1342543DE82EF95)) & 0xFFFFFFFFFFFFFFFF
    with np.errstate(over="ignore"):
        ctr = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(base)) & _MASK
    bits = _splitmix64(_splitmix64(ctr))
    return (bits >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def uniform(seed: int, name: str, shape, lo: float, hi: float) -> np.ndarray:
    n = int(np.prod(shape)) if len(shape) else 1
    u = uniform01(seed, name, n)
    return (lo + (hi - lo) * u).astype(np.float32).reshape(shape)


def default_paddings(upsample_scales):
    """Reference padding rule (articulatory/models/hifigan.py:82-103)."""
    pads = [s // 2 + s % 2 for s in upsample_scales]
    opads = [s % 2 for s in upsample_scales]
    return pads, opads


def generator_param_spec(
    in_channels=80,
    out_channels=1,
    channels=512,
    kernel_size=7,
    upsample_scales=(8, 8, 2, 2),
    upsample_kernel_sizes=(16, 16, 4, 4),
    resblock_kernel_sizes=(3, 7, 11),
    resblock_dilations=((1, 3, 5), (1, 3, 5), (1, 3, 5)),
    use_additional_convs=True,
    bias=True,
    use_weight_norm=True,
    use_ar=False,
    ar_input=512,
    ar_hidden=256,
    ar_output=128,
    use_spk_id=False,
    num_spk=None,
    spk_emb_size=32,
    use_ph=False,
    num_ph=None,
    ph_emb_size=8,
    use_ph_loss=False,
    **_ignored,
):
    """Ordered {state_dict key: shape} of the reference generator for these kwargs.

    Key names and shapes follow what ``HiFiGANGenerator(**kwargs).state_dict()`` yields in the
    reference (articulatory/models/hifigan.py:108-175; verified key-for-key by
    tests/test_oracle_golden.py against the fixture written by oracle/make_golden.py).
    ConvTranspose1d weights are (Cin, Cout, K) and their weight_g is per-*Cin* (dim 0).
    """
    spec = OrderedDict()

    def conv(prefix, w_shape, n_bias, has_bias=True):
        if has_bias:
            spec[prefix + ".bias"] = (n_bias,)
        if use_weight_norm:
            spec[prefix + ".weight_g"] = (w_shape[0], 1, 1)
            spec[prefix + ".weight_v"] = tuple(w_shape)
        else:
            spec[prefix + ".weight"] = tuple(w_shape)

    # torch orders a weight-normed module's params as bias, weight_g, weight_v
    conv("input_conv", (channels, in_channels, kernel_size), channels)
    n_up = len(upsample_kernel_sizes)
    n_blocks = len(resblock_kernel_sizes)
    ups = []
    blocks = []
    for i in range(n_up):
        cin = channels // (2 ** i)
        cout = channels // (2 ** (i + 1))
        ups.append((f"upsamples.{i}.1", (cin, cout, upsample_kernel_sizes[i]), cout))
        for j in range(n_blocks):
            k = resblock_kernel_sizes[j]
            b = i * n_blocks + j
            c1 = [(f"blocks.{b}.convs1.{d}.1", (cout, cout, k), cout) for d in range(len(resblock_dilations[j]))]
            c2 = [(f"blocks.{b}.convs2.{d}.1", (cout, cout, k), cout) for d in range(len(resblock_dilations[j]))]
            blocks.append((c1, c2 if use_additional_convs else []))
    for p, s, nb in ups:
        conv(p, s, nb)
    # only the ResidualBlock convs honour the `bias` flag (residual_block.py:172-205); the input,
    # upsample and output convs are built without one and so always carry a bias (hifigan.py:108-159)
    for c1, c2 in blocks:
        for p, s, nb in c1:
            conv(p, s, nb, bias)
        for p, s, nb in c2:
            conv(p, s, nb, bias)
    c_last = channels // (2 ** n_up)
    conv("output_conv.1", (out_channels, c_last, kernel_size), out_channels)
    if use_ar:
        dims = [ar_input] + [ar_hidden] * 4 + [ar_output]
        for li in range(5):
            spec[f"ar_model.model.{2 * li}.weight"] = (dims[li + 1], dims[li])
            spec[f"ar_model.model.{2 * li}.bias"] = (dims[li + 1],)
    # speaker / phoneme conditioning (hifigan.py:176-189), in the reference's module registration order; Embedding and Linear carry
    # no weight norm (apply_weight_norm only touches Conv1d / ConvTranspose1d, hifigan.py:268-278)
    if use_spk_id:
        spec["spk_emb_mat.weight"] = (num_spk, spk_emb_size)
        spec["spk_fc.weight"] = (in_channels, spk_emb_size)
        spec["spk_fc.bias"] = (in_channels,)
    if use_ph:
        spec["ph_emb_mat.weight"] = (num_ph, ph_emb_size)
    if use_ph_loss:
        spec["ph_fc.weight"] = (num_ph, c_last)
        spec["ph_fc.bias"] = (num_ph,)
    return spec


def synth_state_dict(generator_params: dict, seed: int = 1234, gain: float = 1.0) -> "OrderedDict[str, np.ndarray]":
    """Synthesise a reference-layout generator state_dict as float32 numpy arrays.

    ``weight_v ~ U(-b, b)`` with ``b = gain * sqrt(3 / fan_in)`` (unit-variance-preserving),
    ``weight_g = ||v|| * U(0.8, 1.2)`` so that the weight-norm fold is *not* the identity,
    ``bias ~ U(-0.05, 0.05)``.
    """
    spec = generator_param_spec(**generator_params)
    out = OrderedDict()
    for name, shape in spec.items():
        if name.endswith(".weight_v") or name.endswith(".weight"):
            fan_in = int(np.prod(shape[1:]))
            b = gain * np.sqrt(3.0 / fan_in)
            out[name] = uniform(seed, name, shape, -b, b)
        elif name.endswith(".bias"):
            out[name] = uniform(seed, name, shape, -0.05, 0.05)
    for name, shape in spec.items():
        if name.endswith(".weight_g"):
            v = out[name[: -len("weight_g")] + "weight_v"].astype(np.float64)
            norm = np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(axis=1)).reshape(shape)
            jitter = uniform(seed, name, shape, 0.8, 1.2).astype(np.float64)
            out[name] = (norm * jitter).astype(np.float32)
    # restore spec order
    return OrderedDict((k, out[k]) for k in spec)


GBLOCK_IN = (1, 1, 1, 2, 2, 2, 2, 4, 4, 8)    # divisors of ``channels`` for the ten GBlocks' inputs (gblock_gen.py:63)
GBLOCK_OUT = (1, 1, 2, 2, 2, 2, 4, 4, 8, 8)   # ... and outputs (gblock_gen.py:64)


def gblock_param_spec(
    in_channels=80,
    out_channels=1,
    channels=512,
    kernel_size=7,
    g_scales=(8, 8, 2, 2),
    g_kernel_sizes=(16, 16, 4, 4),
    use_weight_norm=True,
    use_ar=False,
    ar_input=512,
    ar_hidden=256,
    ar_output=128,
    use_spk_id=False,
    num_spk=None,
    spk_emb_size=32,
    **_ignored,
):
    """Ordered {state_dict key: shape} of the reference's ``GBlockGenerator(**kwargs)`` (articulatory/models/gblock_gen.py:17-109; the
    GBlock's layers articulatory/layers/pytorch_layers.py:32-83).  A GBlock's Sequentials hold [ReLU, (Upsample,) conv, ReLU, conv]
    (conv1), [(Upsample,) conv] (res1) and [ReLU, conv, ReLU, conv] (conv2): the conv indices move by one when ``upsample > 1``.
    The GBlocks are built with ``norm=False`` but the generator's apply_weight_norm (gblock_gen.py:161-170) wraps every Conv1d, theirs
    included.  Checked key-for-key against the real class by oracle/make_golden_gblock.py."""
    spec = OrderedDict()

    def conv(prefix, w_shape):
        spec[prefix + ".bias"] = (w_shape[0],)
        if use_weight_norm:
            spec[prefix + ".weight_g"] = (w_shape[0], 1, 1)
            spec[prefix + ".weight_v"] = tuple(w_shape)
        else:  # a plain torch module registers weight before bias
            del spec[prefix + ".bias"]
            spec[prefix + ".weight"] = tuple(w_shape)
            spec[prefix + ".bias"] = (w_shape[0],)

    conv("input_conv", (channels, in_channels, kernel_size))
    for i, (s, k) in enumerate(zip(g_scales, g_kernel_sizes)):
        cin, cout = channels // GBLOCK_IN[i], channels // GBLOCK_OUT[i]
        u = 1 if s > 1 else 0
        base = f"resamples.{i}"
        conv(f"{base}.conv1.{1 + u}", (cout, cin, k))
        conv(f"{base}.conv1.{3 + u}", (cout, cout, k))
        conv(f"{base}.res1.{u}", (cout, cin, 1))
        conv(f"{base}.conv2.1", (cout, cout, k))
        conv(f"{base}.conv2.3", (cout, cout, k))
    conv("output_conv.1", (out_channels, channels // 8, kernel_size))
    if use_ar:
        dims = [ar_input] + [ar_hidden] * 4 + [ar_output]
        for li in range(5):
            spec[f"ar_model.model.{2 * li}.weight"] = (dims[li + 1], dims[li])
            spec[f"ar_model.model.{2 * li}.bias"] = (dims[li + 1],)
    if use_spk_id:
        spec["spk_emb_mat.weight"] = (num_spk, spk_emb_size)
        spec["spk_fc.weight"] = (in_channels, spk_emb_size)
        spec["spk_fc.bias"] = (in_channels,)
    return spec


def _synth_from_spec(spec, seed, gain):
    out = OrderedDict()
    for name, shape in spec.items():
        if name.endswith(".weight_v") or name.endswith(".weight"):
            fan_in = int(np.prod(shape[1:]))
            b = gain * np.sqrt(3.0 / fan_in)
            out[name] = uniform(seed, name, shape, -b, b)
        elif name.endswith(".bias"):
            out[name] = uniform(seed, name, shape, -0.05, 0.05)
    for name, shape in spec.items():
        if name.endswith(".weight_g"):
            v = out[name[: -len("weight_g")] + "weight_v"].astype(np.float64)
            norm = np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(axis=1)).reshape(shape)
            jitter = uniform(seed, name, shape, 0.8, 1.2).astype(np.float64)
            out[name] = (norm * jitter).astype(np.float32)
    return OrderedDict((k, out[k]) for k in spec)


def synth_gblock_state_dict(generator_params: dict, seed: int = 1234, gain: float = 1.0) -> "OrderedDict[str, np.ndarray]":
    """Synthetic reference-layout state_dict of a GBlockGenerator (same recipe as synth_state_dict)."""
    return _synth_from_spec(gblock_param_spec(**generator_params), seed, gain)


def synth_features(batch: int, frames: int, dims: int, seed: int) -> np.ndarray:
    """Synthetic EMA(+pitch) features, (B, T, dims) fp32: N(0,1) with channel 0 ~ U(0,1).

    Mirrors the min-max-normalised pitch channel of the reference's feature files
    (egs/ema/voc1/local/combine_feats.py:42-62).  numpy PCG64, as SURVEY.md §8(d) specifies.
    """
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal((batch, frames, dims)).astype(np.float32)
    x[:, :, 0] = rng.random((batch, frames)).astype(np.float32)
    return x


# ------------------------------------------------------------------------------------------------
# HiFiGANMultiScaleMultiPeriodDiscriminator (reference articulatory/models/hifigan.py:317-825)
# ------------------------------------------------------------------------------------------------
def synth_waveforms(seed, B, T):
    """Waveform pairs for the loss / training fixtures (tests/golden/gold_loss_aux.npz, gold_train_step.npz).  (y_hat, y): band-limited pseudo-speech (a few decaying harmonics + noise) so that the spectra have structure, plus — for the
    LAST sequence — a stretch of exact silence in y_hat longer than the largest frame, which puts whole frames on the magnitude clamps
    (stft_loss.py:40, mel_loss.py:97,100)."""
    t = np.arange(T, dtype=np.float64) / 16000.0
    out = []
    for name in ("y_hat", "y"):
        sig = np.zeros((B, T))
        for b in range(B):
            f0 = 90.0 + 35.0 * b + (7.0 if name == "y" else 0.0)
            amp = uniform(seed, f"{name}.amp.{b}", (8,), 0.02, 0.12).astype(np.float64)
            for h in range(8):
                sig[b] += amp[h] * np.sin(2 * np.pi * f0 * (h + 1) * t + 0.3 * h + b)
        sig += uniform(seed, f"{name}.noise", (B, T), -0.05, 0.05)
        out.append(sig.astype(np.float32))
    y_hat, y = out
    if T >= 2600:
        y_hat[-1, 200:2500] = 0.0
    return y_hat[:, None, :], y[:, None, :]


def synth_train_batch(config, seed, batch):
    """One training batch of a recipe as numpy: {"x": (B, dims, frames), "y": (B, 1, batch_max_steps), "ar": (B, 1, ar_input)} — what the
    reference's collater hands _train_step for the a2w + AR recipes (train.py:1071-1097); the AR context and the window are one
    continuous waveform."""
    gp = config["generator_params"]
    hop = int(np.prod(gp["upsample_scales"]))
    frames = config["batch_max_steps"] // hop
    dims = gp["in_channels"] - gp["ar_output"]
    x = synth_features(batch, frames, dims, seed=seed).transpose(0, 2, 1).copy()
    _, wav = synth_waveforms(seed + 1, batch, gp["ar_input"] + config["batch_max_steps"])
    return {"x": x.astype(np.float32), "y": wav[:, :, gp["ar_input"]:].copy(), "ar": wav[:, :, : gp["ar_input"]].copy()}


DISC_DEFAULTS = dict(
    scales=3,
    scale_downsample_pooling="AvgPool1d",
    scale_downsample_pooling_params={"kernel_size": 4, "stride": 2, "padding": 2},
    scale_discriminator_params={
        "in_channels": 1, "out_channels": 1, "kernel_sizes": [15, 41, 5, 3], "channels": 128, "max_downsample_channels": 1024,
        "max_groups": 16, "bias": True, "downsample_scales": [2, 2, 4, 4, 1], "nonlinear_activation": "LeakyReLU",
        "nonlinear_activation_params": {"negative_slope": 0.1},
    },
    follow_official_norm=True,
    periods=[2, 3, 5, 7, 11],
    period_discriminator_params={
        "in_channels": 1, "out_channels": 1, "kernel_sizes": [5, 3], "channels": 32, "downsample_scales": [3, 3, 3, 3, 1],
        "max_downsample_channels": 1024, "bias": True, "nonlinear_activation": "LeakyReLU",
        "nonlinear_activation_params": {"negative_slope": 0.1}, "use_weight_norm": True, "use_spectral_norm": False,
    },
)


def disc_params(**kw):
    """discriminator_params of a YAML config merged over the reference's defaults (hifigan.py:744-781)."""
    p = {k: (dict(v) if isinstance(v, dict) else v) for k, v in DISC_DEFAULTS.items()}
    for k, v in kw.items():
        if k not in p:
            raise TypeError(f"unexpected discriminator parameter {k!r}")
        p[k] = dict(v) if isinstance(v, dict) else v
    return p


def scale_disc_layers(in_channels=1, out_channels=1, kernel_sizes=(15, 41, 5, 3), channels=128, max_downsample_channels=1024,
                      max_groups=16, bias=True, downsample_scales=(2, 2, 4, 4, 1), **_ignored):
    """Conv1d layers of one HiFiGANScaleDiscriminator (hifigan.py:549-617): dicts of cin, cout, k, stride, groups, act."""
    assert len(kernel_sizes) == 4 and all(k % 2 == 1 for k in kernel_sizes)
    layers = [dict(cin=in_channels, cout=channels, k=kernel_sizes[0], stride=1, groups=1, act=True, bias=bias)]
    in_chs, out_chs, groups = channels, channels, 4
    for s in downsample_scales:
        layers.append(dict(cin=in_chs, cout=out_chs, k=kernel_sizes[1], stride=s, groups=groups, act=True, bias=bias))
        in_chs = out_chs
        out_chs = min(in_chs * 2, max_downsample_channels)
        groups = min(groups * 4, max_groups)
    out_chs = min(in_chs * 2, max_downsample_channels)
    layers.append(dict(cin=in_chs, cout=out_chs, k=kernel_sizes[2], stride=1, groups=1, act=True, bias=bias))
    layers.append(dict(cin=out_chs, cout=out_channels, k=kernel_sizes[3], stride=1, groups=1, act=False, bias=bias))
    for L in layers:
        L["pad"] = (L["k"] - 1) // 2
    return layers


def period_disc_layers(in_channels=1, out_channels=1, kernel_sizes=(5, 3), channels=32, downsample_scales=(3, 3, 3, 3, 1),
                       max_downsample_channels=1024, bias=True, **_ignored):
    """Conv2d (k, 1) layers of one HiFiGANPeriodDiscriminator (hifigan.py:357-389).  NB the output conv's kernel is
    kernel_sizes[1] - 1 with padding (kernel_sizes[1] - 1) // 2 (:383-389), and every Conv2d has a bias whatever ``bias`` says."""
    assert len(kernel_sizes) == 2 and kernel_sizes[0] % 2 == 1 and kernel_sizes[1] % 2 == 1
    layers = []
    in_chs, out_chs = in_channels, channels
    for s in downsample_scales:
        layers.append(dict(cin=in_chs, cout=out_chs, k=kernel_sizes[0], stride=s, groups=1, act=True, bias=True,
                           pad=(kernel_sizes[0] - 1) // 2))
        in_chs = out_chs
        out_chs = min(out_chs * 4, max_downsample_channels)
    layers.append(dict(cin=out_chs, cout=out_channels, k=kernel_sizes[1] - 1, stride=1, groups=1, act=False, bias=True,
                       pad=(kernel_sizes[1] - 1) // 2))
    return layers


def disc_param_spec(**kw):
    """Ordered {state_dict key: shape} of HiFiGANMultiScaleMultiPeriodDiscriminator(**kw) (checked key-for-key against the real
    reference by tests/test_oracle_golden.py through the fixture of oracle/make_golden_disc.py).  The scale discriminators never
    get a norm (their apply_weight_norm / apply_spectral_norm test for Conv2d on a Conv1d stack, hifigan.py:645-663): plain
    weights.  The period discriminators are weight-normed Conv2d (bias, weight_g, weight_v)."""
    p = disc_params(**kw)
    spec = OrderedDict()
    for i in range(p["scales"]):
        layers = scale_disc_layers(**p["scale_discriminator_params"])
        for l, L in enumerate(layers):
            base = f"msd.discriminators.{i}.layers.{l}" + (".0" if L["act"] else "")
            spec[base + ".weight"] = (L["cout"], L["cin"] // L["groups"], L["k"])
            if L["bias"]:
                spec[base + ".bias"] = (L["cout"],)
    pp = p["period_discriminator_params"]
    sn = pp.get("use_spectral_norm", False)
    wn = pp.get("use_weight_norm", True)
    if sn and wn:
        raise ValueError("Either use use_weight_norm or use_spectral_norm.")  # hifigan.py:390-391
    for i, _period in enumerate(p["periods"]):
        layers = period_disc_layers(**pp)
        for l, L in enumerate(layers):
            base = f"mpd.discriminators.{i}." + (f"convs.{l}.0" if L["act"] else "output_conv")
            shape = (L["cout"], L["cin"], L["k"], 1)
            if sn:  # torch.nn.utils.spectral_norm: bias, weight_orig (parameters), weight_u, weight_v (buffers: power-iteration vectors)
                spec[base + ".bias"] = (L["cout"],)
                spec[base + ".weight_orig"] = shape
                spec[base + ".weight_u"] = (L["cout"],)
                spec[base + ".weight_v"] = (L["cin"] * L["k"],)
            elif wn:  # a weight-normed module lists bias first (bias, weight_g, weight_v), a plain one weight, bias
                spec[base + ".bias"] = (L["cout"],)
                spec[base + ".weight_g"] = (L["cout"], 1, 1, 1)
                spec[base + ".weight_v"] = shape
            else:
                spec[base + ".weight"] = shape
                spec[base + ".bias"] = (L["cout"],)
    return spec


def synth_disc_state_dict(discriminator_params: dict, seed: int = 4321, gain: float = 1.0) -> "OrderedDict[str, np.ndarray]":
    """Synthetic discriminator state_dict (same recipe as synth_state_dict)."""
    spec = disc_param_spec(**discriminator_params)
    out = OrderedDict()
    for name, shape in spec.items():
        if len(shape) == 1 and (name.endswith(".weight_u") or name.endswith(".weight_v")):  # spectral norm's unit vectors
            v = uniform(seed, name, shape, -1.0, 1.0).astype(np.float64)
            out[name] = (v / np.sqrt((v * v).sum())).astype(np.float32)
        elif name.endswith(".weight_v") or name.endswith(".weight") or name.endswith(".weight_orig"):
            b = gain * np.sqrt(3.0 / int(np.prod(shape[1:])))
            out[name] = uniform(seed, name, shape, -b, b)
        elif name.endswith(".bias"):
            out[name] = uniform(seed, name, shape, -0.05, 0.05)
    for name, shape in spec.items():
        if name.endswith(".weight_g"):
            v = out[name[: -len("weight_g")] + "weight_v"].astype(np.float64)
            norm = np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(axis=1)).reshape(shape)
            out[name] = (norm * uniform(seed, name, shape, 0.8, 1.2).astype(np.float64)).astype(np.float32)
    return OrderedDict((k, out[k]) for k in spec)


# ------------------------------------------------------------------------------------------------
# BiGRU, the speech-to-EMA inversion model (reference articulatory/models/pytorch_models.py:22-123)
# ------------------------------------------------------------------------------------------------
def bigru_param_spec(in_channels=80, hidden_size=256, out_channels=1, use_tanh=False, **_ignored):
    """Ordered {state_dict key: shape} of the reference's ``BiGRU(**kwargs)`` without use_ar / use_spk_emb: torch.nn.GRU lists a
    direction's weight_ih, weight_hh, bias_ih, bias_hh and then the reverse direction's; BatchNorm1d its parameters, then its buffers.
    Checked key-for-key against the real class by tools/make_golden_bigru.py (tests/golden/gold_bigru_keys.txt)."""
    spec = OrderedDict()
    H = hidden_size
    for name, cin in (("gru1", in_channels), ("gru2", 2 * H)):
        for sfx in ("", "_reverse"):
            spec[f"{name}.weight_ih_l0{sfx}"] = (3 * H, cin)
            spec[f"{name}.weight_hh_l0{sfx}"] = (3 * H, H)
            spec[f"{name}.bias_ih_l0{sfx}"] = (3 * H,)
            spec[f"{name}.bias_hh_l0{sfx}"] = (3 * H,)
    spec["fc1.0.weight"] = (128, 2 * H)
    spec["fc1.0.bias"] = (128,)
    spec["bn.weight"] = (128,)
    spec["bn.bias"] = (128,)
    spec["bn.running_mean"] = (128,)
    spec["bn.running_var"] = (128,)
    spec["bn.num_batches_tracked"] = ()
    fc2 = "fc2.0" if use_tanh else "fc2"
    spec[fc2 + ".weight"] = (out_channels, 128)
    spec[fc2 + ".bias"] = (out_channels,)
    return spec


def synth_bigru_state_dict(params: dict, seed: int = 1234, gain: float = 1.0) -> "OrderedDict[str, np.ndarray]":
    """Synthetic reference-layout state_dict of a BiGRU from the same name-keyed generator as the other specs: matrices
    U(+-gain * sqrt(3 / fan_in)), biases U(+-0.05), a batch norm that is not the identity (running_var in [0.5, 1.5], weight in
    [0.8, 1.2], running_mean and bias in +-0.3), num_batches_tracked an int64 scalar.  gain 1 keeps the recurrence well conditioned:
    at gain 2 an fp32 and a float64 run of the reference already differ by 3e-6 .. 8e-6 of max|y|, at gain 4 completely."""
    out = OrderedDict()
    for name, shape in bigru_param_spec(**params).items():
        if name == "bn.num_batches_tracked":
            out[name] = np.array(1000, dtype=np.int64)
        elif name == "bn.running_var":
            out[name] = uniform(seed, name, shape, 0.5, 1.5)
        elif name == "bn.weight":
            out[name] = uniform(seed, name, shape, 0.8, 1.2)
        elif name in ("bn.running_mean", "bn.bias"):
            out[name] = uniform(seed, name, shape, -0.3, 0.3)
        elif len(shape) == 2:
            b = gain * np.sqrt(3.0 / shape[1])
            out[name] = uniform(seed, name, shape, -b, b)
        else:
            out[name] = uniform(seed, name, shape, -0.05, 0.05)
    return out


# ------------------------------------------------------------------------------------------------
# BiGRU training: the dropout masks of libhificar's counter-based generator (csrc/hificar_bigru_train_kernels.hip.h: BigruDrop)
# ------------------------------------------------------------------------------------------------
BIGRU_DROPOUT_SITES = {"gru1": 0, "gru2": 1, "fc1": 2}  # the output each nn.Dropout of the reference acts on (pytorch_models.py:65-68)


def bigru_dropout_mask(seed: int, offset: int, site, shape, p: float) -> np.ndarray:
    """The factor (0, or 1 / (1 - p) in float32) of every element of the (B, T, C) tensor at ``site`` for training forward number ``offset``
    of a model seeded with ``seed``: element e (row-major index) is kept when u(seed, offset, site, e) >= p, u = the top 24 bits of
    splitmix64(key + e) / 2^24 with key = splitmix64(seed ^ splitmix64(4 offset + site)).  ``p = 0`` gives all ones and draws nothing."""
    site = BIGRU_DROPOUT_SITES[site] if isinstance(site, str) else int(site)
    n = int(np.prod(shape))
    p32 = np.float32(p)
    if not p32 > 0:
        return np.ones(shape, dtype=np.float32)
    inner = _splitmix64(np.array([(4 * int(offset) + site) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))
    key = _splitmix64(np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64) ^ inner)
    with np.errstate(over="ignore"):
        bits = _splitmix64((np.arange(n, dtype=np.uint64) + key) & _MASK)
    u = (bits >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    scale = np.float32(1.0) / (np.float32(1.0) - p32)
    return np.where(u >= p32, scale, np.float32(0.0)).astype(np.float32).reshape(shape)


# ------------------------------------------------------------------------------------------------
# Transformer, the feature-to-feature encoder (reference articulatory/models/transformer.py:21-105)
# ------------------------------------------------------------------------------------------------
XFMR_DROPOUT_SITES = {"attn": 0, "dropout1": 1, "dropout": 2, "dropout2": 3}  # per encoder layer l: site 4 l + these


def xfmr_dropout_mask(seed: int, offset: int, site: int, shape_or_band, p: float) -> np.ndarray:
    """The dropout factors (0, or 1 / (1 - p) in float32) of the Transformer's training forward number ``offset`` at ``site`` = 4 l + {0: the
    attention probabilities, 1: dropout1, 2: the feed-forward's hidden rows, 3: dropout2} of encoder layer l (csrc/hificar_xfmr_kernels.hip.h:
    XfmrDrop): the BiGRU generator's draw, u = the top 24 bits of splitmix64(key + e) / 2^24 kept when u >= p, with
    key = splitmix64(seed ^ splitmix64(128 offset + site)).

    Sites 1-3: ``shape_or_band`` is the (B, T, C) shape and e the row-major index.  Site 0: ``shape_or_band`` is (B, T) and the result is the
    dense (B, 8, T, T) mask whose entry (b, h, q, k) with |k - q| <= 99 is element e = ((b 8 + h) T + q) 199 + (k - q + 99); entries outside the
    band are 1 (no such probability exists).  ``p = 0`` gives all ones and draws nothing."""
    site = int(site)
    band = site % 4 == 0
    if band:
        B, T = (int(v) for v in shape_or_band)
        shape = (B, 8, T, T)
    else:
        shape = tuple(int(v) for v in shape_or_band)
    p32 = np.float32(p)
    if not p32 > 0:
        return np.ones(shape, dtype=np.float32)
    inner = _splitmix64(np.array([(128 * int(offset) + site) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))
    key = _splitmix64(np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64) ^ inner)
    if band:
        q = np.arange(T, dtype=np.int64)[:, None]
        k = np.arange(T, dtype=np.int64)[None, :]
        rel = k - q + 99
        inband = (rel >= 0) & (rel < 199)
        row = (np.arange(B * 8, dtype=np.int64).reshape(B, 8, 1, 1) * T + q[None, None]) * 199
        e = (row + np.where(inband, rel, 0)[None, None]).astype(np.uint64)
    else:
        e = np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)
    with np.errstate(over="ignore"):
        bits = _splitmix64((e + key) & _MASK)
    u = (bits >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    scale = np.float32(1.0) / (np.float32(1.0) - p32)
    out = np.where(u >= p32, scale, np.float32(0.0)).astype(np.float32)
    if band:
        out = np.where(inband[None, None], out, np.float32(1.0)).astype(np.float32)
    return out


def transformer_param_spec(in_channels=8, out_channels=80, elayers=6, hidden_dim=768, **_ignored):
    """Ordered {state_dict key: shape} of the reference's ``Transformer(**kwargs)`` without extra_art / num_ph: a ResBlock lists conv1, bn1
    (parameters, then buffers), conv2, bn2 and, where it changes the width, residual_path and res_norm; an encoder layer its attention's
    w_q, w_k, w_v, w_o and table, linear1, linear2, norm1, norm2.  Checked key-for-key against the real class by
    tools/make_golden_transformer.py (tests/golden/gold_transformer_keys.txt)."""
    spec = OrderedDict()
    F, d = hidden_dim, hidden_dim // 8

    def bn(base):
        for t in ("weight", "bias", "running_mean", "running_var"):
            spec[f"{base}.{t}"] = (F,)
        spec[f"{base}.num_batches_tracked"] = ()

    for i in range(3):
        cin = in_channels if i == 0 else F
        b = f"conv_blocks.{i}"
        spec[b + ".conv1.weight"] = (F, cin, 3)
        spec[b + ".conv1.bias"] = (F,)
        bn(b + ".bn1")
        spec[b + ".conv2.weight"] = (F, F, 3)
        spec[b + ".conv2.bias"] = (F,)
        bn(b + ".bn2")
        if cin != F:
            spec[b + ".residual_path.weight"] = (F, cin, 1)
            spec[b + ".residual_path.bias"] = (F,)
            bn(b + ".res_norm")
    spec["w_raw_in.weight"] = (F, F)
    spec["w_raw_in.bias"] = (F,)
    for l in range(elayers):
        b = f"transformer.layers.{l}"
        for w in ("w_q", "w_k", "w_v"):
            spec[f"{b}.self_attn.{w}"] = (8, F, d)
        spec[b + ".self_attn.w_o"] = (8, d, F)
        spec[b + ".self_attn.relative_positional.embeddings"] = (8, 199, d, 1)
        spec[b + ".linear1.weight"] = (3072, F)
        spec[b + ".linear1.bias"] = (3072,)
        spec[b + ".linear2.weight"] = (F, 3072)
        spec[b + ".linear2.bias"] = (F,)
        for n in ("norm1", "norm2"):
            spec[f"{b}.{n}.weight"] = (F,)
            spec[f"{b}.{n}.bias"] = (F,)
    spec["w_out.weight"] = (out_channels, F)
    spec["w_out.bias"] = (out_channels,)
    return spec


def synth_transformer_state_dict(params: dict, seed: int = 1234, gain: float = 1.0) -> "OrderedDict[str, np.ndarray]":
    """Synthetic reference-layout state_dict of a Transformer from the same name-keyed generator as the other specs: matrices and conv
    kernels U(+-gain * sqrt(3 / fan_in)) (w_q / w_k / w_v: fan_in = hidden_dim, w_o: 8 d; the positional table U(+-sqrt(3 / d)), the
    reference's initial spread), biases U(+-0.05), batch norms that are not the identity (running_var in [0.5, 2], weight in [0.8, 1.2],
    running_mean and bias in +-0.3), layer norms with weight in [0.8, 1.2], num_batches_tracked an int64 scalar."""
    out = OrderedDict()
    for name, shape in transformer_param_spec(**params).items():
        leaf = name.rsplit(".", 1)[-1]
        norm = any(t in name for t in (".bn1.", ".bn2.", ".res_norm.", ".norm1.", ".norm2."))
        if leaf == "num_batches_tracked":
            out[name] = np.array(1000, dtype=np.int64)
        elif leaf == "running_var":
            out[name] = uniform(seed, name, shape, 0.5, 2.0)
        elif norm and leaf == "weight":
            out[name] = uniform(seed, name, shape, 0.8, 1.2)
        elif leaf == "running_mean" or (norm and leaf == "bias" and ".norm" not in name):
            out[name] = uniform(seed, name, shape, -0.3, 0.3)
        elif leaf == "embeddings":
            b = np.sqrt(3.0 / shape[2])
            out[name] = uniform(seed, name, shape, -b, b)
        elif leaf in ("w_q", "w_k", "w_v"):
            b = gain * np.sqrt(3.0 / shape[1])
            out[name] = uniform(seed, name, shape, -b, b)
        elif leaf == "w_o":
            b = gain * np.sqrt(3.0 / (shape[0] * shape[1]))
            out[name] = uniform(seed, name, shape, -b, b)
        elif len(shape) >= 2:
            b = gain * np.sqrt(3.0 / int(np.prod(shape[1:])))
            out[name] = uniform(seed, name, shape, -b, b)
        else:
            out[name] = uniform(seed, name, shape, -0.05, 0.05)
    return out


# ---- HuBERT ("large" family) ----------------------------------------------------------------------------------------------------------
HUBERT_CONV_KERNEL = (10, 3, 3, 3, 3, 2, 2)
HUBERT_CONV_STRIDE = (5, 2, 2, 2, 2, 2, 2)


def hubert_param_spec(config):
    """Ordered {state_dict key: shape} of the ``transformers`` library's ``HubertModel`` for a "large"-family configuration (layer-norm
    extractor, stable layer norm, weight-normed positional conv in its parametrized form); ``config``: a mapping with the keys of its
    ``config.json``.  ``masked_spec_embed`` exists when the configuration's mask probabilities say so, as in the library.  Checked
    key-for-key against the real class by tools/make_golden_hubert.py (tests/golden/gold_hubert_keys.txt)."""
    spec = OrderedDict()
    dims = list(config.get("conv_dim", (512,) * 7))
    kernels = list(config.get("conv_kernel", HUBERT_CONV_KERNEL))
    H, I = config.get("hidden_size", 1024), config.get("intermediate_size", 4096)
    taps, groups = config.get("num_conv_pos_embeddings", 128), config.get("num_conv_pos_embedding_groups", 16)
    if config.get("mask_time_prob", 0.05) > 0.0 or config.get("mask_feature_prob", 0.0) > 0.0:
        spec["masked_spec_embed"] = (H,)
    for i, (c, k) in enumerate(zip(dims, kernels)):
        b = f"feature_extractor.conv_layers.{i}"
        spec[b + ".conv.weight"] = (c, 1 if i == 0 else dims[i - 1], k)
        if config.get("conv_bias", True):
            spec[b + ".conv.bias"] = (c,)
        spec[b + ".layer_norm.weight"] = (c,)
        spec[b + ".layer_norm.bias"] = (c,)
    spec["feature_projection.layer_norm.weight"] = (dims[-1],)
    spec["feature_projection.layer_norm.bias"] = (dims[-1],)
    spec["feature_projection.projection.weight"] = (H, dims[-1])
    spec["feature_projection.projection.bias"] = (H,)
    spec["encoder.pos_conv_embed.conv.bias"] = (H,)
    spec["encoder.pos_conv_embed.conv.parametrizations.weight.original0"] = (1, 1, taps)
    spec["encoder.pos_conv_embed.conv.parametrizations.weight.original1"] = (H, H // groups, taps)
    spec["encoder.layer_norm.weight"] = (H,)
    spec["encoder.layer_norm.bias"] = (H,)
    for l in range(config.get("num_hidden_layers", 24)):
        b = f"encoder.layers.{l}"
        for w in ("k_proj", "v_proj", "q_proj", "out_proj"):
            spec[f"{b}.attention.{w}.weight"] = (H, H)
            spec[f"{b}.attention.{w}.bias"] = (H,)
        spec[b + ".layer_norm.weight"] = (H,)
        spec[b + ".layer_norm.bias"] = (H,)
        spec[b + ".feed_forward.intermediate_dense.weight"] = (I, H)
        spec[b + ".feed_forward.intermediate_dense.bias"] = (I,)
        spec[b + ".feed_forward.output_dense.weight"] = (H, I)
        spec[b + ".feed_forward.output_dense.bias"] = (H,)
        spec[b + ".final_layer_norm.weight"] = (H,)
        spec[b + ".final_layer_norm.bias"] = (H,)
    return spec


def synth_hubert_state_dict(config, seed: int = 1234, gain: float = 1.0) -> "OrderedDict[str, np.ndarray]":
    """Synthetic ``HubertModel``-layout state_dict from the name-keyed generator of the other specs: matrices and conv kernels
    U(+-gain * sqrt(3 / fan_in)), biases U(+-0.05), layer norms away from the identity (weight in [0.8, 1.2], bias in +-0.3), the
    positional conv's weight_g (original0) in [0.5, 1.5] * sqrt(hidden_size / 128) — each tap's kernel is g v / ||v|| over ALL its
    hidden x group elements — and masked_spec_embed in [0, 1) as the library draws it."""
    out = OrderedDict()
    H = config.get("hidden_size", 1024)
    for name, shape in hubert_param_spec(config).items():
        leaf = name.rsplit(".", 1)[-1]
        if name == "masked_spec_embed":
            out[name] = uniform(seed, name, shape, 0.0, 1.0)
        elif "layer_norm" in name:
            out[name] = uniform(seed, name, shape, 0.8, 1.2) if leaf == "weight" else uniform(seed, name, shape, -0.3, 0.3)
        elif leaf == "original0":
            s = float(np.sqrt(H / 128.0))
            out[name] = uniform(seed, name, shape, 0.5 * s, 1.5 * s)
        elif len(shape) >= 2:
            b = gain * np.sqrt(3.0 / int(np.prod(shape[1:])))
            out[name] = uniform(seed, name, shape, -b, b)
        else:
            out[name] = uniform(seed, name, shape, -0.05, 0.05)
    return out


# ---- WavLM ("large" family): HuBERT-large with the gated relative position bias -----------------------------------------------------------
def wavlm_param_spec(config):
    """Ordered {state_dict key: shape} of the ``transformers`` library's ``WavLMModel`` for a "large"-family configuration: ``hubert_param_spec``
    with, in every layer's attention, ``gru_rel_pos_const`` (1, heads, 1, 1) in front of the projections and ``gru_rel_pos_linear`` (8, 64)
    behind them, and layer 0's ``rel_attn_embed`` (num_buckets, heads) last.  Checked key-for-key against the real class by
    tools/make_golden_wavlm.py (tests/golden/gold_wavlm_keys.txt)."""
    heads, nb = config.get("num_attention_heads", 16), config.get("num_buckets", 320)
    H = config.get("hidden_size", 1024)
    spec = OrderedDict()
    for k, shape in hubert_param_spec(config).items():
        if k.endswith(".attention.k_proj.weight"):
            spec[k[:-len("k_proj.weight")] + "gru_rel_pos_const"] = (1, heads, 1, 1)
        spec[k] = shape
        if k.endswith(".attention.out_proj.bias"):
            b = k[:-len("out_proj.bias")]
            spec[b + "gru_rel_pos_linear.weight"] = (8, H // heads)
            spec[b + "gru_rel_pos_linear.bias"] = (8,)
            if b == "encoder.layers.0.attention.":
                spec[b + "rel_attn_embed.weight"] = (nb, heads)
    return spec


def synth_wavlm_state_dict(config, seed: int = 1234, gain: float = 1.0) -> "OrderedDict[str, np.ndarray]":
    """``synth_hubert_state_dict`` in ``WavLMModel``'s layout.  ``rel_attn_embed`` is N(0, 1) (Box-Muller over the name-keyed generator), as
    large as the scaled dot products, ``gru_rel_pos_const`` U(0.5, 1.5), and the gate's ``Linear`` U(+-0.5 sqrt(3 / 64)) with biases
    U(+-0.05): over a LayerNorm's output the two four-sums have a deviation near one, so the sigmoids stay off their rails and the gates spread
    over most of their range — a wrong bucket, sign or gate moves the output by orders of magnitude more than any tolerance."""
    base = synth_hubert_state_dict(config, seed=seed, gain=gain)
    out = OrderedDict()
    for name, shape in wavlm_param_spec(config).items():
        if name in base:
            out[name] = base[name]
        elif name.endswith("rel_attn_embed.weight"):
            n = int(np.prod(shape))
            u1 = uniform01(seed, name + "#r", n).astype(np.float64)
            u2 = uniform01(seed, name + "#a", n).astype(np.float64)
            z = np.sqrt(-2.0 * np.log(np.maximum(u1, 2.0 ** -40))) * np.cos(2.0 * np.pi * u2)
            out[name] = z.reshape(shape).astype(np.float32)
        elif name.endswith("gru_rel_pos_const"):
            out[name] = uniform(seed, name, shape, 0.5, 1.5)
        elif name.endswith("gru_rel_pos_linear.weight"):
            b = 0.5 * np.sqrt(3.0 / shape[1])
            out[name] = uniform(seed, name, shape, -b, b)
        else:
            out[name] = uniform(seed, name, shape, -0.05, 0.05)
    return out
