#!/usr/bin/env python3
"""tests/golden/gold_arloop_cond.npz: the chunked AR loop of speaker- / phoneme-conditioned models, from the REAL reference generator.

The reference's own driver cannot run such a model (decode.py:72 calls ``model(cin, ar=prev_samples)`` only), so this script drives
the reference's unmodified ``HiFiGANGenerator`` chunk by chunk with the driver's chunking and feedback (decode.py:54-83):

    chunks x[i:i+n], i = 0, n, 2n, ... (the last one shorter and kept); prev = zeros, then the last ar_input samples of the previous
    chunk's output; chunk output = forward(x[i:i+n].T[None], spk_id=[s], ar=prev, ph=p[None, i:i+n]); result = the concatenation

Same rules as oracle/make_golden.py, whose ``import_reference()`` is used (the reference is imported at run time, in the build
container only; only data is written).  Every case is also run in float64: a case whose fp32 loop deviates from it by more than 1e-5
of max|y| is ill conditioned as a yardstick and is not written.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_arloop_cond.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))

from make_golden import import_reference, yaml_generator_params  # noqa: E402

CHUNK = 25
LENGTHS = (60, 260)  # both end in a ragged 10-frame chunk
MAX_F32_DEVIATION = 1e-5


def chunked_loop(forward, x, chunk, ar_input, spk=None, ph=None):
    """The loop of the module docstring over one utterance x (T, C); forward(c, spk_id=, ar=, ph=) -> (1, 1, hop * frames)."""
    import torch

    prev = torch.zeros((1, 1, ar_input), dtype=x.dtype)
    outs = []
    for i in range(0, len(x), chunk):
        kw = {}
        if spk is not None:
            kw["spk_id"] = torch.tensor([spk], dtype=torch.int64)
        if ph is not None:
            kw["ph"] = ph[None, i:i + chunk]
        y = forward(x[i:i + chunk].t()[None], ar=prev, **kw)
        outs.append(y[0, 0])
        prev = y[:, :, -ar_input:]
    return torch.cat(outs)


def main():
    import copy

    import torch

    from articulatory_amd.utils.synth import synth_features, synth_state_dict

    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref_models, _, _ = import_reference()
    full = yaml_generator_params("e2w_hifigan.yaml")["generator_params"]

    def build(params, seed):
        g = ref_models.HiFiGANGenerator(**params)
        sd = synth_state_dict(params, seed=seed)
        assert list(g.state_dict().keys()) == list(sd.keys()), "param spec disagrees with the reference's state_dict keys"
        g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        g.remove_weight_norm()
        return g.eval()

    cases = {
        "spk": (dict(full, channels=128, use_spk_id=True, num_spk=5, spk_emb_size=32), 4321),
        "ph": (dict(full, channels=128, in_channels=13 + 128 + 8, use_ph=True, num_ph=11, ph_emb_size=8), 4323),
    }
    res = {"chunk_frames": np.array(CHUNK), "lengths": np.array(LENGTHS)}
    rng = np.random.Generator(np.random.PCG64(701))
    for k, (tag, (params, seed)) in enumerate(sorted(cases.items())):
        g = build(params, seed)
        g64 = copy.deepcopy(g).double()
        feats = synth_features(len(LENGTHS), max(LENGTHS), 13, seed=710 + k)
        for u, T in enumerate(LENGTHS):
            x = torch.from_numpy(feats[u, :T].copy())
            spk = int(rng.integers(0, params["num_spk"])) if params.get("use_spk_id") else None
            ph = torch.from_numpy(rng.integers(0, params["num_ph"], size=T).astype(np.int64)) if params.get("use_ph") else None
            with torch.no_grad():
                y = chunked_loop(g, x, CHUNK, params["ar_input"], spk, ph)
                y64 = chunked_loop(g64, x.double(), CHUNK, params["ar_input"], spk, ph)
            dev = float((y.double() - y64).abs().max() / y64.abs().max())
            print(f"{tag} T={T}: max|y|={float(y64.abs().max()):.4f}  fp32 vs fp64 loop {dev:.3e}")
            if not dev <= MAX_F32_DEVIATION:
                raise SystemExit(f"{tag} T={T}: fp32 deviates from fp64 by {dev:.3e} > {MAX_F32_DEVIATION}: not written")
            res[f"{tag}_x{T}"] = x.numpy()
            res[f"{tag}_out{T}"] = y.numpy()
            res[f"{tag}_f32_dev{T}"] = np.array(dev)
            if spk is not None:
                res[f"{tag}_spk{T}"] = np.array(spk, dtype=np.int64)
            if ph is not None:
                res[f"{tag}_ph{T}"] = ph.numpy()
    path = os.path.join(REPO, "tests", "golden", "gold_arloop_cond.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
