#!/usr/bin/env python3
"""Speech -> EMA by a linear regression on a speech model's hidden states: the reference's ``egs/ema/voc1/local/linear_inference.py``
(``hidden_states[9]`` of ``wavlm_large`` through a fitted ``sklearn`` regression), on the device from the wav to the prediction.

    python -m articulatory_amd.bin.linear_inference WAVS LINEAR OUTDIR --ssl-model DIR [--layer 9] [--batch-size N]
                                                    [--ssl-precision {f32,bf16x3}] [--dry-run]

``WAVS``: a directory of ``<utt>.wav`` files, a kaldi-style ``wav.scp`` or one wav file (mono PCM_16 at 16 kHz; another rate or a file under
400 samples is refused by name — nothing is resampled).  ``LINEAR``: the head, a ``.joblib`` (a fitted ``LinearRegression`` or ``Ridge``) or an
``.npz`` with ``coef`` / ``intercept`` (``features.LinearHead.load``).  ``--ssl-model DIR``: a WavLM or HuBERT model of the large family in the
``transformers`` layout (``features.ssl_encoder_from_pretrained``); ``--layer N`` takes ``hidden_states[N]`` (layers N and above are not run;
default 9, the reference's), ``--layer -1`` the last hidden state.  ``OUTDIR/<utt>.npy`` is (frames, out) float32 at 50 Hz: the reference
does not interpolate, and neither does this.  Every utterance is computed as if alone, so any ``--batch-size`` writes the same bytes.
``--dry-run`` reads the configuration and the wav headers alone, prints the plan as one JSON line and needs no GPU.
"""

import argparse
import json
import logging
import os

import numpy as np
import torch

from articulatory_amd.bin.decode import length_batches
from articulatory_amd.bin.predict_ema import SSL_RATE, check_ssl_wavs, list_wavs, read_wav, wav_info


def get_parser():
    parser = argparse.ArgumentParser(description="Predict EMA from wavs with a speech model's hidden states and a fitted linear regression.")
    parser.add_argument("wavs", type=str, help="directory of <utt>.wav files (mono PCM_16, 16 kHz), a wav.scp, or one wav file")
    parser.add_argument("linear", type=str, help="the head: a .joblib (fitted sklearn LinearRegression / Ridge) or an .npz with coef / intercept")
    parser.add_argument("outdir", type=str, help="directory to save <utt>.npy, each (frames, out) at 50 Hz")
    parser.add_argument("--ssl-model", type=str, required=True,
                        help="directory of a WavLM or HuBERT model (large family; transformers layout: config.json + model.safetensors | pytorch_model.bin)")
    parser.add_argument("--layer", type=int, default=9, help="take hidden_states[N] (0 .. layers - 1; default 9); -1: the last hidden state")
    parser.add_argument("--batch-size", type=int, default=1, help="utterances per device call (any lengths)")
    parser.add_argument("--ssl-precision", default=None, choices=("f32", "bf16x3", "bf16x3a"),
                        help="arithmetic of the encoder's GEMMs; default: f32 (bf16x3a: HuBERT only)")
    parser.add_argument("--verbose", type=int, default=1, help="logging level. higher is more logging. (default=1)")
    parser.add_argument("--dry-run", default=False, action="store_true", help="print the plan as one JSON line and exit (no GPU needed)")
    return parser


def predict_linear(encoder, head, pairs, outdir, device, layer=9, batch_size=1):
    """(utt_id, wav path) pairs -> ``outdir/<utt_id>.npy`` (frames, out).  Batches of similar lengths; per batch the padded waveforms go to
    the device in one copy and stay there through ``encoder`` and ``head`` up to the prediction.  Returns the number of utterances."""
    n = 0
    with torch.no_grad():
        wavs = ((u, read_wav(p)[0]) for u, p in pairs)
        for batch in length_batches(wavs, max(1, batch_size)):
            lens = [len(y) for _, y in batch]
            padded = np.zeros((len(batch), max(lens)), dtype=np.float32)
            for i, (_, y) in enumerate(batch):
                padded[i, :lens[i]] = y
            feats, frames = encoder(torch.from_numpy(padded).to(device), lens, layer=layer)
            yb = head(feats, frames)
            counts = [encoder.frames(l) for l in lens]
            for i, (utt_id, _) in enumerate(batch):
                np.save(os.path.join(outdir, f"{utt_id}.npy"), yb[i, :, :counts[i]].transpose(0, 1).cpu().numpy())
                n += 1
    return n


def main(argv=None):
    from articulatory_amd._native import hubert_frames
    from articulatory_amd.features import LinearHead, ssl_encoder_class

    args = get_parser().parse_args(argv)
    level = logging.DEBUG if args.verbose > 1 else logging.INFO if args.verbose > 0 else logging.WARN
    logging.basicConfig(level=level, format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s")
    if os.path.isfile(args.wavs) and args.wavs.endswith(".wav"):
        pairs = [(os.path.basename(args.wavs)[: -len(".wav")], args.wavs)]
    else:
        pairs = list_wavs(args.wavs)
    encoder_class = ssl_encoder_class(args.ssl_model)  # HuBERT or WavLM, by config.json's model_type
    with open(os.path.join(args.ssl_model, "config.json")) as f:
        config = encoder_class._check_config(json.load(f))
    encoder_class._check_precision(args.ssl_precision or "f32")  # (WavLM refuses bf16x3a: before anything loads)
    if not -1 <= args.layer < config["num_hidden_layers"]:
        raise ValueError(f"--layer {args.layer} outside -1 .. {config['num_hidden_layers'] - 1}")
    info = {p: wav_info(p) for _, p in pairs}
    check_ssl_wavs(pairs, info)
    if args.dry_run:
        print(json.dumps({"encoder": encoder_class._NAME.lower(), "ssl_model": args.ssl_model, "layer": args.layer,
                          "layers_run": config["num_hidden_layers"] if args.layer < 0 else args.layer, "num_hidden_layers": config["num_hidden_layers"],
                          "ssl_precision": args.ssl_precision or "f32", "hidden_size": config["hidden_size"], "linear": args.linear,
                          "batch_size": args.batch_size, "rates": [SSL_RATE], "frame_rate": 50, "utterances": [u for u, _ in pairs],
                          "samples": int(sum(info[p][1] for _, p in pairs)),
                          "frames": int(sum(hubert_frames(info[p][1]) for _, p in pairs))}), flush=True)
        return
    if not torch.cuda.is_available():
        raise RuntimeError("linear_inference: no GPU visible; this package has no CPU inference path")
    head = LinearHead.load(args.linear)
    if head.in_features != config["hidden_size"]:
        raise ValueError(f"{args.linear}: the head takes {head.in_features} features, the speech model's hidden_size is {config['hidden_size']}")
    if not os.path.exists(args.outdir):
        os.makedirs(args.outdir)
    device = torch.device("cuda")
    encoder = encoder_class.from_pretrained(args.ssl_model, precision=args.ssl_precision or "f32").to(device)
    logging.info(f"Loaded the speech model ({encoder_class._NAME}) from {args.ssl_model}.")
    n = predict_linear(encoder, head.to(device), pairs, args.outdir, device, layer=args.layer, batch_size=args.batch_size)
    logging.info(f"Finished prediction of {n} utterances.")


if __name__ == "__main__":
    main()
