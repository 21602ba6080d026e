#!/usr/bin/env python3
"""Golden vectors of the WavLM encoder from the ``transformers`` library's ``WavLMModel`` (offline: random-weight construction from a
``WavLMConfig``, the synthetic weights loaded with strict=True, run in float64 on CPU).

    HF_HUB_OFFLINE=1 python tools/make_golden_wavlm.py

writes tests/golden/gold_wavlm.npz — for the tiny configuration (tools/make_golden_hubert.py's ``TINY`` plus ``num_buckets=32,
max_bucket_distance=24``: exact buckets under 8, logarithmic ones for 8 .. 23, saturated from 24 on) last_hidden_state and every
hidden_states[k] at 1, 2 and 65 frames, and last_hidden_state at 129 frames — and tests/golden/gold_wavlm_keys.txt, the state_dict's key /
shape list at the tiny and the large configuration.  Inputs and weights are regenerated from seeds, not stored.  The file's job is to pin
the numpy oracle (tests/wavlm_oracle.py), which the GPU tests then use at every length.
"""

import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from articulatory_amd.utils.synth import synth_wavlm_state_dict, wavlm_param_spec  # noqa: E402
from tests import hubert_oracle as O  # noqa: E402
from tools.make_golden_hubert import LARGE as HUBERT_LARGE, TINY as HUBERT_TINY  # noqa: E402

TINY = dict(HUBERT_TINY, num_buckets=32, max_bucket_distance=24)
LARGE = dict(HUBERT_LARGE, num_buckets=320, max_bucket_distance=800)
SEED = 4242
FULL = (400, 720, 400 + 320 * 64)   # 1, 2 and 65 frames
LAST_ONLY = (400 + 320 * 128,)      # 129 frames: three key blocks, every bucket region on both signs


def library_model(config, meta=False):
    from transformers import WavLMConfig, WavLMModel

    cfg = WavLMConfig(**config, attn_implementation="eager")
    if meta:
        with torch.device("meta"):
            return WavLMModel(cfg)
    return WavLMModel(cfg).double().eval()


def library_forward(model, wav):
    x = torch.from_numpy(O.normalize(wav))[None]
    with torch.no_grad():
        return model(x, output_hidden_states=True)


def load_synthetic(model, config, seed=SEED):
    sd = synth_wavlm_state_dict(config, seed=seed)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items()}, strict=True)
    return sd


def main():
    out = {}
    model = library_model(TINY)
    load_synthetic(model, TINY)
    for L in FULL + LAST_ONLY:
        r = library_forward(model, O.synth_wav(SEED + L, L))
        out[f"L{L}.last_hidden_state"] = r.last_hidden_state[0].numpy()
        if L in LAST_ONLY:
            continue
        for k, h in enumerate(r.hidden_states):
            out[f"L{L}.hidden_states.{k}"] = h[0].numpy()
    path = os.path.join(REPO, "tests", "golden", "gold_wavlm.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")
    lines = []
    for name, config in (("tiny", TINY), ("large", LARGE)):
        real = library_model(config, meta=True).state_dict()
        spec = wavlm_param_spec(config)
        assert list(real) == list(spec), [k for k in real if k not in spec] + [k for k in spec if k not in real]
        for k, v in real.items():
            assert tuple(v.shape) == tuple(spec[k]), (k, tuple(v.shape), spec[k])
            lines.append(f"{name} {k} {','.join(str(s) for s in v.shape)}")
    with open(os.path.join(REPO, "tests", "golden", "gold_wavlm_keys.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(len(lines), "keys")


if __name__ == "__main__":
    main()
