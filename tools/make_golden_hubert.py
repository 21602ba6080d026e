#!/usr/bin/env python3
"""Golden vectors of the HuBERT encoder from the ``transformers`` library's ``HubertModel`` (offline: random-weight construction from a
``HubertConfig``, the synthetic weights loaded with strict=True, run in float64 on CPU).

    HF_HUB_OFFLINE=1 python tools/make_golden_hubert.py

writes tests/golden/gold_hubert.npz — for the tiny configuration (tests/hubert_oracle users: ``TINY``) and each length of ``FULL``:
last_hidden_state, every hidden_states[k], extract_features, the output of extractor layer 0 (lengths of ``TAP0`` only: it is 64 floats per
200-Hz position) and of the positional conv; for ``LAST_ONLY`` the last hidden state alone.  Inputs and weights are regenerated from
seeds (tests/hubert_oracle.synth_wav, utils/synth.synth_hubert_state_dict), not stored.  The lengths are a subset of those the GPU tests run:
float64 tensors of all of them would not fit the 1 MB a committed file may have, and the file's job is to pin the numpy oracle, which the
GPU tests then use at every length — and tests/golden/gold_hubert_keys.txt, the state_dict's key / shape list at the tiny and the large
configuration.
"""

import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from articulatory_amd.utils.synth import hubert_param_spec, synth_hubert_state_dict  # noqa: E402
from tests import hubert_oracle as O  # noqa: E402

TINY = dict(conv_dim=[64] * 7, conv_kernel=list(O.KERNELS), conv_stride=list(O.STRIDES), hidden_size=128, num_attention_heads=2, intermediate_size=256,
            num_hidden_layers=2, conv_bias=True, feat_extract_norm="layer", do_stable_layer_norm=True, feat_proj_layer_norm=True,
            layer_norm_eps=1e-5, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, hidden_act="gelu",
            feat_extract_activation="gelu", mask_time_prob=0.05, mask_feature_prob=0.0)
LARGE = dict(TINY, conv_dim=[512] * 7, hidden_size=1024, num_attention_heads=16, intermediate_size=4096, num_hidden_layers=24)
SEED = 4242
FULL = (400, 719, 720, 400 + 320 * 64)  # 1, 1, 2 and 65 frames
TAP0 = (400, 719, 720)
LAST_ONLY = (400 + 320 * 128,)          # 129 frames: three key blocks, a sequence longer than the positional kernel


def library_model(config, meta=False):
    from transformers import HubertConfig, HubertModel

    cfg = HubertConfig(**config, attn_implementation="eager")
    if meta:
        with torch.device("meta"):
            return HubertModel(cfg)
    return HubertModel(cfg).double().eval()


def main():
    out = {}
    sd = synth_hubert_state_dict(TINY, seed=SEED)
    model = library_model(TINY)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items()}, strict=True)
    taps = {}
    model.feature_extractor.conv_layers[0].register_forward_hook(lambda m, i, o: taps.__setitem__("extractor.0", o))
    model.encoder.pos_conv_embed.register_forward_hook(lambda m, i, o: taps.__setitem__("pos_conv", o))
    for L in FULL + LAST_ONLY:
        wav = O.synth_wav(SEED + L, L)
        x = torch.from_numpy(O.normalize(wav))[None]
        with torch.no_grad():
            r = model(x, output_hidden_states=True)
        out[f"L{L}.last_hidden_state"] = r.last_hidden_state[0].numpy()
        if L in LAST_ONLY:
            continue
        for k, h in enumerate(r.hidden_states):
            out[f"L{L}.hidden_states.{k}"] = h[0].numpy()
        with torch.no_grad():
            out[f"L{L}.extract_features"] = model.feature_extractor(x)[0].transpose(0, 1).numpy()
        out[f"L{L}.pos_conv"] = taps["pos_conv"][0].numpy()
        if L in TAP0:
            out[f"L{L}.extractor.0"] = taps["extractor.0"][0].transpose(0, 1).numpy()
    path = os.path.join(REPO, "tests", "golden", "gold_hubert.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")
    lines = []
    for name, config in (("tiny", TINY), ("large", LARGE)):
        real = library_model(config, meta=True).state_dict()
        spec = hubert_param_spec(config)
        assert list(real) == list(spec), [k for k in real if k not in spec] + [k for k in spec if k not in real]
        for k, v in real.items():
            assert tuple(v.shape) == tuple(spec[k]), (k, tuple(v.shape), spec[k])
            lines.append(f"{name} {k} {','.join(str(s) for s in v.shape)}")
    with open(os.path.join(REPO, "tests", "golden", "gold_hubert_keys.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(len(lines), "keys")


if __name__ == "__main__":
    main()
