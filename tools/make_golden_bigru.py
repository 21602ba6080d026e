#!/usr/bin/env python3
"""tests/golden/gold_bigru.npz and gold_bigru_keys.txt: the BiGRU inversion model, from the REAL reference class.

Same rules as oracle/make_golden.py, whose ``import_reference()`` is used (the reference is imported at run time, in the build
container only; only data is written).  The weights are NOT stored: ``synth_bigru_state_dict(params, seed)`` regenerates them, loaded here
with the reference's own ``load_state_dict`` (strict), so the key list is checked against the real class.

Cases (Cin, H, out): (1024, 256, 18) at T = 400; (13, 256, 12) with use_tanh at T = 500; (80, 64, 12) at T = 1 and T = 300 — plus, on the
small model, ``.inference()`` with registered statistics and a ragged batch in which every utterance is run alone.

Admission condition: every case is also run in float64, and is written only if the fp32 run is within 2e-6 of max|y| of it (one tenth of
the project's exact-fp32 bar of 2e-5); otherwise the tool stops.  The deviation is stored as ``<case>_f32_dev``.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_bigru.py
"""
import copy
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))

from make_golden import import_reference  # noqa: E402

MAX_F32_DEVIATION = 2e-6
GAIN = 1.0
CASES = {  # tag: (params, seed, frame counts)
    "full": (dict(in_channels=1024, hidden_size=256, out_channels=18, use_tanh=False), 5101, (400,)),
    "mfcc": (dict(in_channels=13, hidden_size=256, out_channels=12, use_tanh=True), 5102, (500,)),
    "small": (dict(in_channels=80, hidden_size=64, out_channels=12, use_tanh=False), 5103, (1, 300)),
}
RAGGED = (300, 1, 137, 300)


def main():
    import torch

    from articulatory_amd.utils.synth import synth_bigru_state_dict, uniform

    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref_models, _, _ = import_reference()
    res, keys = {}, None

    def admit(tag, y32, y64):
        dev = float((y32.double() - y64).abs().max() / y64.abs().max())
        if not dev <= MAX_F32_DEVIATION:
            raise SystemExit(f"{tag}: fp32 deviates from float64 by {dev:.3g} of max|y| (> {MAX_F32_DEVIATION}): not a yardstick")
        res[tag + "_f32_dev"] = np.array(dev)
        print(f"{tag}: shape {tuple(y32.shape)}, max|y| {float(y64.abs().max()):.4f}, f32 dev {dev:.3g}")
        return y32.numpy()

    for tag, (params, seed, frames) in CASES.items():
        m = ref_models.BiGRU(**params)
        sd = synth_bigru_state_dict(params, seed=seed, gain=GAIN)
        assert list(m.state_dict().keys()) == list(sd.keys()), "param spec disagrees with the reference's state_dict keys"
        for k, v in m.state_dict().items():
            assert tuple(v.shape) == tuple(sd[k].shape) and (v.dtype == torch.int64) == (sd[k].dtype == np.int64), k
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        m.eval()
        m64 = copy.deepcopy(m).double()
        if tag == "full":
            keys = list(sd.keys())
        with torch.no_grad():
            for T in frames:
                x = uniform(seed, f"x.{T}", (1, params["in_channels"], T), -1.0, 1.0)
                case = f"{tag}_T{T}"
                res[case + "_x"] = x
                res[case + "_y"] = admit(case, m(torch.from_numpy(x)), m64(torch.from_numpy(x).double()))
            if tag == "small":
                # inference() with statistics: (T, C) in, (T, out) back (pytorch_models.py:86-105)
                C = params["in_channels"]
                stats = np.stack([uniform(seed, "stats.mean", (C,), -0.5, 0.5), uniform(seed, "stats.scale", (C,), 0.5, 2.0)])
                for mm in (m, m64):
                    mm.register_buffer("mean", torch.from_numpy(stats[0]).to(next(mm.parameters()).dtype))
                    mm.register_buffer("scale", torch.from_numpy(stats[1]).to(next(mm.parameters()).dtype))
                c = uniform(seed, "inference.c", (200, C), -2.0, 2.0)
                res["small_stats"] = stats
                res["small_inf_c"] = c
                res["small_inf_y"] = admit("small_inf", m.inference(torch.from_numpy(c)), m64.inference(torch.from_numpy(c).double()))
                res["small_inf_raw_y"] = admit("small_inf_raw", m.inference(torch.from_numpy(c), normalize_before=False),
                                               m64.inference(torch.from_numpy(c).double(), normalize_before=False))
                # ragged batch: every utterance alone, rows past its length zero
                xr = uniform(seed, "ragged.x", (len(RAGGED), C, max(RAGGED)), -1.0, 1.0)
                yr = torch.zeros((len(RAGGED), params["out_channels"], max(RAGGED)))
                yr64 = yr.double()
                for b, n in enumerate(RAGGED):
                    xr[b, :, n:] = 0.0
                    yr[b, :, :n] = m(torch.from_numpy(xr[b:b + 1, :, :n]))[0]
                    yr64[b, :, :n] = m64(torch.from_numpy(xr[b:b + 1, :, :n]).double())[0]
                res["small_ragged_lengths"] = np.array(RAGGED, dtype=np.int32)
                res["small_ragged_x"] = xr
                res["small_ragged_y"] = admit("small_ragged", yr, yr64)
    for tag, (params, seed, _) in CASES.items():
        res[tag + "_params"] = np.array([params["in_channels"], params["hidden_size"], params["out_channels"], int(params["use_tanh"]), seed])
    gold = os.path.join(REPO, "tests", "golden")
    # the (1024, 256, 18) case's input alone is 1.6 MB of fp32, over the limit for a committed file: the tests regenerate it from
    # (seed, name) with the same name-keyed generator (``uniform(seed, "x.400", ...)``) and only its output is stored
    del res["full_T400_x"]
    np.savez_compressed(os.path.join(gold, "gold_bigru.npz"), **res)
    with open(os.path.join(gold, "gold_bigru_keys.txt"), "w") as f:
        f.write("\n".join(keys) + "\n")
    print("wrote", os.path.getsize(os.path.join(gold, "gold_bigru.npz")), "bytes")


if __name__ == "__main__":
    main()
