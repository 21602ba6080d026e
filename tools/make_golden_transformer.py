#!/usr/bin/env python3
"""tests/golden/gold_transformer.npz, gold_transformer_taps.npz and gold_transformer_keys.txt: the Transformer feature model, from the REAL
reference class.

Same rules as oracle/make_golden.py, whose ``import_reference()`` is used (the reference is imported at run time, in the build container
only; only data is written).  The weights are NOT stored: ``synth_transformer_state_dict(params, seed)`` regenerates them, loaded here with
the reference's own ``load_state_dict`` (strict), so the key list is checked against the real class.  The inputs are not stored either: the
tests regenerate them by name with the same generator (``uniform(seed, "x.<T>", ...)``).

The reference's own ``Transformer.forward`` does not run on a current torch (``nn.TransformerEncoder.forward`` looks for a ``batch_first``
attribute its ``MultiHeadAttention`` does not have); with ``norm=None`` the encoder is nothing but its layers in order, so this tool applies
``conv_blocks``, ``w_raw_in``, every module of ``transformer.layers`` (their own sub-modules, in eval mode) and ``w_out`` itself.

Cases: the default size (12 -> 80, hidden 768, 6 layers) at T = 400; a small model (80 -> 18, hidden 128, 2 layers) at T = 1, 100, 101 and
260 with taps (rows (1, T, 128)) after conv_blocks, after w_raw_in, after each layer's attention sub-block (post-norm1) and after each layer;
the small model's ``.inference()``; and a ragged batch of lengths (260, 1, 137, 260) in which every utterance is run alone.  The taps of the
T = 260 case go to gold_transformer_taps.npz (one file with all of them would pass the size limit for a committed file).

Admission condition: every array is also computed in float64, and is written only if the fp32 run is within 2e-6 of max|y| of it (one tenth
of the project's exact-fp32 bar of 2e-5); otherwise the tool stops.  The deviation is stored as ``<name>_f32_dev``.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_transformer.py
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
CASES = {  # tag: (params, seed, frame counts)
    "default": (dict(in_channels=12, out_channels=80, elayers=6, hidden_dim=768), 6101, (400,)),
    "small": (dict(in_channels=80, out_channels=18, elayers=2, hidden_dim=128), 6102, (1, 100, 101, 260)),
}
RAGGED = (260, 1, 137, 260)
TAPS_FILE_T = 260


def run(m, x, taps=None):
    """Transformer.forward (transformer.py:55-77) with the encoder written out as its layers (pytorch_layers.py:162-177, eval mode)."""
    taps = taps if taps is not None else {}
    h = m.conv_blocks(x).transpose(1, 2)
    taps["conv_blocks"] = h
    h = m.w_raw_in(h)
    taps["w_raw_in"] = h
    h = h.transpose(0, 1)  # (T, B, F)
    for l, layer in enumerate(m.transformer.layers):
        h = layer.norm1(h + layer.dropout1(layer.self_attn(h)))
        taps[f"layers.{l}.norm1"] = h.transpose(0, 1)
        h = layer.norm2(h + layer.dropout2(layer.linear2(layer.dropout(layer.activation(layer.linear1(h))))))
        taps[f"layers.{l}"] = h.transpose(0, 1)
    return m.w_out(h.transpose(0, 1)).transpose(1, 2)


def main():
    import torch

    from articulatory_amd.utils.synth import synth_transformer_state_dict, uniform

    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref_models, _, _ = import_reference()
    res, res_taps, keys = {}, {}, None

    def admit(tag, y32, y64, into=None):
        dev = float((y32.double() - y64).abs().max() / y64.abs().max())
        if not dev <= MAX_F32_DEVIATION:
            raise SystemExit(f"{tag}: fp32 deviates from float64 by {dev:.3g} of max|y| (> {MAX_F32_DEVIATION}): not a yardstick")
        into = res if into is None else into
        into[tag + "_f32_dev"] = np.array(dev)
        print(f"{tag}: shape {tuple(y32.shape)}, max|y| {float(y64.abs().max()):.4f}, f32 dev {dev:.3g}")
        return y32.contiguous().numpy()

    for tag, (params, seed, frames) in CASES.items():
        m = ref_models.Transformer(**params)
        sd = synth_transformer_state_dict(params, seed=seed)
        assert list(m.state_dict().keys()) == list(sd.keys()), "param spec disagrees with the reference's state_dict keys"
        for k, v in m.state_dict().items():
            assert tuple(v.shape) == tuple(sd[k].shape) and (v.dtype == torch.int64) == (sd[k].dtype == np.int64), k
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        m.eval()
        m64 = copy.deepcopy(m).double()
        if tag == "default":
            keys = list(sd.keys())
        with torch.no_grad():
            for T in frames:
                x = torch.from_numpy(uniform(seed, f"x.{T}", (1, params["in_channels"], T), -1.0, 1.0))
                case = f"{tag}_T{T}"
                t32, t64 = {}, {}
                res[case + "_y"] = admit(case, run(m, x, t32), run(m64, x.double(), t64))
                if tag == "small":
                    into = res_taps if T == TAPS_FILE_T else res
                    for name in t32:
                        into[f"{case}_tap_{name}"] = admit(f"{case}_tap_{name}", t32[name], t64[name], into)
            if tag == "small":
                # inference(): (T, C) in, (T, out) back (transformer.py:100-105), with forward standing for the written-out encoder
                C = params["in_channels"]
                for mm in (m, m64):
                    mm.forward = (lambda mod: lambda x: run(mod, x))(mm)
                c = torch.from_numpy(uniform(seed, "inference.c", (200, C), -2.0, 2.0))
                res["small_inf_y"] = admit("small_inf", m.inference(c), m64.inference(c.double()))
                # ragged batch: every utterance alone, frames past its length zero
                xr = uniform(seed, "ragged.x", (len(RAGGED), C, max(RAGGED)), -1.0, 1.0)
                yr = torch.zeros((len(RAGGED), params["out_channels"], max(RAGGED)))
                yr64 = yr.double()
                for b, n in enumerate(RAGGED):
                    yr[b, :, :n] = run(m, torch.from_numpy(xr[b:b + 1, :, :n]))[0]
                    yr64[b, :, :n] = run(m64, torch.from_numpy(xr[b:b + 1, :, :n]).double())[0]
                res["small_ragged_lengths"] = np.array(RAGGED, dtype=np.int32)
                res["small_ragged_y"] = admit("small_ragged", yr, yr64)
    for tag, (params, seed, _) in CASES.items():
        res[tag + "_params"] = np.array([params["in_channels"], params["out_channels"], params["elayers"], params["hidden_dim"], seed])
    gold = os.path.join(REPO, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "gold_transformer.npz"), **res)
    np.savez_compressed(os.path.join(gold, "gold_transformer_taps.npz"), **res_taps)
    with open(os.path.join(gold, "gold_transformer_keys.txt"), "w") as f:
        f.write("\n".join(keys) + "\n")
    for n in ("gold_transformer.npz", "gold_transformer_taps.npz"):
        print("wrote", n, os.path.getsize(os.path.join(gold, n)), "bytes")


if __name__ == "__main__":
    main()
