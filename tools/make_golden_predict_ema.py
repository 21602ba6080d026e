#!/usr/bin/env python3
"""tests/golden/gold_predict_ema.npz: the reference's speech-to-EMA driver (egs/ema/voc1/local/predict_ema.py:86-101) on low-rate features,
from the REAL reference classes.

Same rules as tools/make_golden_bigru.py: ``oracle/make_golden.import_reference()`` imports the reference at run time, in the build container
only, and only data is written.  Neither weights nor inputs are stored: ``synth_bigru_state_dict`` / ``synth_transformer_state_dict`` and the
name-keyed ``uniform(seed, name, ...)`` regenerate them.  predict_ema.py itself cannot be imported (it loads s3prl and librosa at module
level), so its lines 86-101 are restated here with the reference's own ``BiGRU`` / ``Transformer``, torch's own ``F.interpolate(size=len *
interp_factor, mode='linear', align_corners=False)`` and ``scipy.stats.zscore(feat, axis=None)``, then ``model.inference(feat,
normalize_before=False)``.  The Transformer runs with its encoder written out, as in tools/make_golden_transformer.py (whose ``run`` is used).

Cases: BiGRU ``small`` (80 -> 12, H 64) at f = 4 with Tl in (1, 2, 33, 75), at f = 2 with Tl = 50 and at f = 3 with Tl = 11; BiGRU ``mfcc``
(13 -> 12, tanh, H 64) z-scored at T = 130; a ragged batch of low-rate lengths (75, 1, 34, 0) at f = 4, every utterance alone; Transformer
``small`` (80 -> 18, hidden 128, 2 layers) at f = 4 with Tl in (1, 33) and z-scored at T = 100.

Admission condition: every case is computed in float32 as the reference does and in float64; the float64 values are stored, and only if
the fp32 run is within 2e-6 of max|y| of them (one tenth of the project's exact-fp32 bar of 2e-5); otherwise the tool stops.
The deviation is stored as ``<case>_f32_dev``.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_predict_ema.py
"""
import copy
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from make_golden import import_reference  # noqa: E402

MAX_F32_DEVIATION = 2e-6
BIGRU = {  # tag: (params, seed)
    "small": (dict(in_channels=80, hidden_size=64, out_channels=12, use_tanh=False), 7101),
    "mfcc": (dict(in_channels=13, hidden_size=64, out_channels=12, use_tanh=True), 7102),
}
XFMR = {"small": (dict(in_channels=80, out_channels=18, elayers=2, hidden_dim=128), 7103)}
# (model, tag, interp_factor, zscore, low-rate frames)
CASES = [("bigru", "small", 4, False, 1), ("bigru", "small", 4, False, 2), ("bigru", "small", 4, False, 33), ("bigru", "small", 4, False, 75),
         ("bigru", "small", 2, False, 50), ("bigru", "small", 3, False, 11), ("bigru", "mfcc", 1, True, 130),
         ("xfmr", "small", 4, False, 1), ("xfmr", "small", 4, False, 33), ("xfmr", "small", 1, True, 100)]
RAGGED = (75, 1, 34, 0)
RAGGED_FACTOR = 4


def case_name(model, tag, f, z, Tl):
    return f"{model}_{tag}_f{f}{'_z' if z else ''}_Tl{Tl}"


def input_range(z):
    """z-scored cases get an input off centre (mean 1, spread 4), the others the models' usual (-1, 1)."""
    return (-1.0, 3.0) if z else (-1.0, 1.0)


def predict(model, feat, f, z, dtype):
    """predict_ema.py:86-101 for one utterance: feat (frames, channels) numpy -> (f * frames, out) tensor."""
    import torch
    from scipy import stats

    if z:  # wav2mfcc's last statement (:34), on the (channels, frames) matrix librosa returns
        feat = stats.zscore(np.asarray(feat, dtype=np.float64 if dtype == torch.float64 else np.float32).T, axis=None).T
    feature = torch.from_numpy(np.ascontiguousarray(feat)).to(dtype)
    if f != 1:
        target_length = len(feature) * f
        feature = torch.nn.functional.interpolate(feature.unsqueeze(0).transpose(1, 2), size=target_length, mode='linear', align_corners=False)
        feature = feature.transpose(1, 2).squeeze(0)
    return model.inference(feature, normalize_before=False)


def main():
    import torch

    from articulatory_amd.utils.synth import synth_bigru_state_dict, synth_transformer_state_dict, uniform
    from make_golden_transformer import run

    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref_models, _, _ = import_reference()
    res = {}

    def admit(tag, y32, y64):
        dev = float((y32.double() - y64).abs().max() / y64.abs().max())
        if not dev <= MAX_F32_DEVIATION:
            raise SystemExit(f"{tag}: fp32 deviates from float64 by {dev:.3g} of max|y| (> {MAX_F32_DEVIATION}): not a yardstick")
        res[tag + "_f32_dev"] = np.array(dev)
        print(f"{tag}: shape {tuple(y64.shape)}, max|y| {float(y64.abs().max()):.4f}, f32 dev {dev:.3g}")
        return y64.contiguous().numpy()

    models = {}
    for tag, (params, seed) in BIGRU.items():
        m = ref_models.BiGRU(**params)
        sd = synth_bigru_state_dict(params, seed=seed, gain=1.0)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        models["bigru", tag] = (m.eval(), copy.deepcopy(m).double().eval(), params, seed)
        res[f"bigru_{tag}_params"] = np.array([params["in_channels"], params["hidden_size"], params["out_channels"], int(params["use_tanh"]), seed])
    for tag, (params, seed) in XFMR.items():
        m = ref_models.Transformer(**params)
        sd = synth_transformer_state_dict(params, seed=seed)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        m.eval()
        m64 = copy.deepcopy(m).double().eval()
        for mm in (m, m64):  # (the reference's own encoder call does not run on a current torch: make_golden_transformer.py)
            mm.forward = (lambda mod: lambda x: run(mod, x))(mm)
        models["xfmr", tag] = (m, m64, params, seed)
        res[f"xfmr_{tag}_params"] = np.array([params["in_channels"], params["out_channels"], params["elayers"], params["hidden_dim"], seed])

    with torch.no_grad():
        for model, tag, f, z, Tl in CASES:
            m, m64, params, seed = models[model, tag]
            name = case_name(model, tag, f, z, Tl)
            lo, hi = input_range(z)
            feat = uniform(seed, f"feat.{name}", (Tl, params["in_channels"]), lo, hi)  # (frames, channels), as the speech model gives them
            res[name + "_y"] = admit(name, predict(m, feat, f, z, torch.float32), predict(m64, feat, f, z, torch.float64))
        m, m64, params, seed = models["bigru", "small"]
        xr = uniform(seed, "ragged.feat", (len(RAGGED), max(RAGGED), params["in_channels"]), -1.0, 1.0)
        T = RAGGED_FACTOR * max(RAGGED)
        yr, yr64 = torch.zeros((len(RAGGED), T, params["out_channels"])), torch.zeros((len(RAGGED), T, params["out_channels"]), dtype=torch.float64)
        for b, n in enumerate(RAGGED):
            if n:
                yr[b, :RAGGED_FACTOR * n] = predict(m, xr[b, :n], RAGGED_FACTOR, False, torch.float32)
                yr64[b, :RAGGED_FACTOR * n] = predict(m64, xr[b, :n], RAGGED_FACTOR, False, torch.float64)
        res["bigru_small_ragged_lengths"] = np.array(RAGGED, dtype=np.int32)
        res["bigru_small_ragged_factor"] = np.array(RAGGED_FACTOR)
        res["bigru_small_ragged_y"] = admit("bigru_small_ragged", yr, yr64)
    path = os.path.join(REPO, "tests", "golden", "gold_predict_ema.npz")
    np.savez_compressed(path, **res)
    print("wrote", os.path.getsize(path), "bytes,", len(res), "keys")


if __name__ == "__main__":
    main()
