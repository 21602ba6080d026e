#!/usr/bin/env python3
"""Decoding drivers — counterparts of the reference's articulatory/bin/decode.py.

* ``ar_loop`` (reference decode.py:31-100): the chunked autoregressive driver.  The reference loop is
  batch-1 Python with one generator forward and one host round trip of ``prev_samples`` per chunk; here
  the whole non-WSOLA loop (all chunks, PastFCEncoder included, feedback taken straight from the output
  buffer) is enqueued on the device by ONE C-ABI call.  ``ar_loop_batch`` runs B equal-length utterances
  side by side and ``ar_loop_ragged`` B utterances of different lengths (each exactly as if it were alone),
  which the reference cannot.  The WSOLA variant (``do_wsola``: half-overlapping chunks,
  decode.py:84-100) is a per-chunk loop over ``model.forward`` as in the reference, since each chunk's
  context comes from the *middle* of the previous chunk.  Speaker- / phoneme-conditioned models (``spk_id=`` / ``ph=``; the
  reference's loop has neither and cannot run one) go through the same calls: every chunk's forward is the reference's
  ``forward(c, spk_id=, ar=prev, ph=)`` (hifigan.py:212-220) with the utterance's speaker and the chunk's slice of its phoneme row.
* ``main`` (reference decode.py:103-358, console script ``articulatory-decode``): same flags, config
  merge, scp / dump-dir inputs (``.npy`` features), ``--normalize-before``, PCM_16 ``<utt>_gen.wav``
  outputs and RTF report, for the a2w dataset modes of the HiFi-GAN / HiFi-CAR generator — and, for the feature-to-feature modes
  ``art`` / ``a2m`` of a non-AR model (the BiGRU inversion model), ``model.inference`` saved as ``<utt>_gen.npy`` (decode.py:338-350).
"""

import argparse
import glob
import logging
import os
import time

import numpy as np
import torch
import yaml

from articulatory_amd.utils.scp import is_supported, load_scp_value


def _chunk_frames(config, params_key="generator_params"):
    in_chunk_len = int(config["batch_max_steps"] / config["hop_size"])
    past_out_len = config[params_key]["ar_input"]
    return in_chunk_len, past_out_len


def _given(**kw):
    """The keyword arguments that were given: an unconditioned model is called exactly as before."""
    return {k: v for k, v in kw.items() if v is not None}


def _spk_tensor(spk_ids, device):
    return None if spk_ids is None else torch.as_tensor([int(s) for s in spk_ids], dtype=torch.int64, device=device)


def _ph_tensor(phs, lens, device):
    """list of (T_i,) phoneme rows -> (B, T_max) zero-padded, like the features."""
    if phs is None:
        return None
    out = torch.zeros((len(phs), max(lens)), dtype=torch.int64, device=device)
    for i, p in enumerate(phs):
        p = torch.as_tensor(p).reshape(-1)
        if p.shape[0] != lens[i]:
            raise ValueError(f"utterance {i}: {p.shape[0]} phoneme indices for {lens[i]} frames")
        out[i, :lens[i]] = p.to(device)
    return out


def ar_loop(model, x, config, do_wsola=False, modality=None, generator2=False, spk_id=None, ph=None):
    """x: (art_len, num_feats) tensor on the model's device -> (audio_len,) tensor
    (``do_wsola``: -> (list of chunk waveforms, list of chunk inputs), as the reference returns).
    ``spk_id``: the utterance's speaker index (use_spk_id models); ``ph``: its (art_len,) phoneme indices (use_ph models)."""
    if modality is not None or generator2:
        raise NotImplementedError("ar_loop: multi-modality / generator2 variants are not built (SURVEY.md §8 f3)")
    if config.get("dataset_mode", "a2w") == "w2a":
        raise NotImplementedError("ar_loop: w2a (inversion) models are out of scope")
    in_chunk_len, past_out_len = _chunk_frames(config)
    if x.dim() == 1:
        x = x.unsqueeze(1)
    if not do_wsola:
        c = x.transpose(0, 1).unsqueeze(0)  # (1, num_feats, art_len)
        return model.ar_synthesis(c, in_chunk_len, **_given(spk_id=None if spk_id is None else _spk_tensor([spk_id], x.device),
                                                            ph=_ph_tensor(None if ph is None else [ph], [x.shape[0]], x.device)))[0]

    # decode.py:84-100: chunks start every in_chunk_len/2 frames and are in_chunk_len (+ extra_art) long
    extra_art = config["generator_params"]["extra_art"]
    audio_chunk_len = config["batch_max_steps"]
    assert in_chunk_len % 2 == 0
    starts = list(range(0, len(x), int(in_chunk_len / 2)))
    ins = [x[i:i + in_chunk_len + int(extra_art)] for i in starts]
    cond = {}
    if spk_id is not None:
        cond["spk_id"] = _spk_tensor([spk_id], x.device)
    if ph is not None:
        ph = _ph_tensor([ph], [x.shape[0]], x.device)
    prev_samples = torch.zeros((1, 1, past_out_len), dtype=x.dtype, device=x.device)
    outs = []
    for art_i, art in enumerate(ins):
        if ph is not None:
            cond["ph"] = ph[:, starts[art_i]:starts[art_i] + len(art)]
        signal = model(art.unsqueeze(0).permute(0, 2, 1), ar=prev_samples, **cond)  # (1, 1, audio_chunk_length)
        outs.append(signal[0][0])
        if art_i < len(ins) - 1:
            prev_samples = signal[:, :, int(audio_chunk_len / 2) - past_out_len:int(audio_chunk_len / 2)]
            assert prev_samples.shape[2] == past_out_len
    return outs, ins


def ar_loop_batch(model, xs, config, spk_id=None, ph=None):
    """xs: (B, art_len, num_feats) equal-length utterances -> (B, audio_len).  ``spk_id`` (B,) / ``ph`` (B, art_len) as in ``ar_loop``."""
    in_chunk_len, _ = _chunk_frames(config)
    return model.ar_synthesis(xs.permute(0, 2, 1), in_chunk_len, **_given(spk_id=spk_id, ph=ph))


def pad_utterances(xs):
    """list of (T_i, C) tensors -> ((B, T_max, C) zero-padded tensor, [T_i])."""
    lens = [int(x.shape[0]) for x in xs]
    out = torch.zeros((len(xs), max(lens), xs[0].shape[1]), dtype=xs[0].dtype, device=xs[0].device)
    for i, x in enumerate(xs):
        out[i, :lens[i]] = x
    return out, lens


def ar_loop_ragged(model, xs, config, batch=64, spk_id=None, ph=None):
    """xs: list of (T_i, num_feats) tensors of any lengths -> list of (hop * T_i,) waveforms; every utterance gets the
    result of ``ar_loop`` on it alone (its own short tail chunk included).  One device call for the whole list: at most
    ``batch`` utterances are in flight and a finished one is replaced by the next (longest first, so the tail is short).
    ``spk_id``: list of speaker indices, ``ph``: list of (T_i,) phoneme rows, one per utterance."""
    in_chunk_len, _ = _chunk_frames(config)
    order = sorted(range(len(xs)), key=lambda i: -int(xs[i].shape[0]))
    padded, lens = pad_utterances([xs[i] for i in order])
    y = model.ar_synthesis_packed(padded.permute(0, 2, 1), in_chunk_len, lens, batch=batch,
                                  **_given(spk_id=None if spk_id is None else _spk_tensor([spk_id[i] for i in order], padded.device),
                                           ph=None if ph is None else _ph_tensor([ph[i] for i in order], lens, padded.device)))
    hop = y.shape[1] // padded.shape[1]
    out = [None] * len(xs)
    for k, i in enumerate(order):
        out[i] = y[k, :hop * lens[k]]
    return out


def windows(items, n):
    """Consecutive groups of up to n items of an iterable (bounded memory for a whole-dataset decode)."""
    buf = []
    for it in items:
        buf.append(it)
        if len(buf) >= n:
            yield buf
            buf = []
    if buf:
        yield buf


def length_batches(items, batch_size, window=8):
    """Group (key, tensor) items into batches of <= batch_size with similar lengths: sort a window of
    ``window * batch_size`` items by length (bounded memory, little padding), cut it into batches."""
    buf = []
    for it in items:
        buf.append(it)
        if len(buf) >= window * batch_size:
            buf.sort(key=lambda kv: kv[1].shape[0])
            while buf:
                yield buf[:batch_size]
                buf = buf[batch_size:]
    buf.sort(key=lambda kv: kv[1].shape[0])
    while buf:
        yield buf[:batch_size]
        buf = buf[batch_size:]


# ----------------------------------------------------------------------------------------------
# articulatory-decode counterpart
# ----------------------------------------------------------------------------------------------
_A2W_MODES = ("default", "m2w", "a2w", "a2w_pcd")
_FEAT_MODES = ("art", "a2m")  # feature -> feature (decode.py:338-350), non-AR models only; w2a / ph2m / ph2a are not built


def list_features(feats_scp=None, dumpdir=None, fmt="npy"):
    """(utt_id, path) pairs of a kaldi-style ``utt_id path.npy`` scp (the reference's NpyScpLoader, utils/utils.py:240-291)
    or of a dump dir of ``<utt_id>-feats.npy`` files (decode.py:207-222).  Nothing is loaded here."""
    if (feats_scp is not None) == (dumpdir is not None):
        raise ValueError("Please specify either --dumpdir or --feats-scp.")
    pairs = []
    if feats_scp is not None:
        with open(feats_scp) as f:
            for line in f:
                parts = line.strip().split()
                if len(parts) < 2:
                    continue
                if not is_supported(parts[1]):
                    raise ValueError("Not supported feats.scp type.")
                pairs.append((parts[0], parts[1]))
    else:
        if fmt == "hdf5":  # decode.py:210-212: <utt_id>.h5 files holding a "feats" dataset
            for path in sorted(glob.glob(os.path.join(dumpdir, "**", "*.h5"), recursive=True)):
                pairs.append((os.path.splitext(os.path.basename(path))[0], path))
        elif fmt == "npy":
            for path in sorted(glob.glob(os.path.join(dumpdir, "**", "*-feats.npy"), recursive=True)):
                pairs.append((os.path.basename(path)[: -len("-feats.npy")], path))
        else:
            raise ValueError("Support only hdf5 or npy format.")
    return pairs


def _load(path):
    return load_scp_value(path)  # .npy, .h5[:dataset], .ark:offset (articulatory_amd/utils/scp.py)


def npy_frames(path):
    """Frame count of a (T, C) feature file (.npy: from its header alone, no data is read)."""
    if not path.endswith(".npy"):
        return int(_load(path).shape[0])
    return int(np.load(path, mmap_mode="r").shape[0])


def load_features(pairs):
    """(utt_id, path) pairs -> (utt_id, (T, C) ndarray), one utterance at a time, as the reference's loop streams them."""
    for utt_id, path in pairs:
        yield utt_id, _load(path)


def iter_features(feats_scp=None, dumpdir=None, fmt="npy"):
    """(utt_id, (T, C) ndarray) pairs, loaded lazily."""
    return load_features(list_features(feats_scp, dumpdir, fmt))


def add_conditioning_arguments(parser):
    """--utt2spk / --spk-list / --ph-scp: who speaks / which phoneme each frame carries, for use_spk_id / use_ph checkpoints (not in the
    reference, whose decoders cannot run such a model)."""
    parser.add_argument("--utt2spk", default=None, type=str, help="'utt_id speaker' lines: the speaker of every utterance (use_spk_id models)")
    parser.add_argument("--spk-list", default=None, type=str,
                        help="one speaker per line, in the training set's order (the index is the model's spk_id); "
                             "default: the sorted speakers of --utt2spk, as training derives them")
    parser.add_argument("--ph-scp", default=None, type=str,
                        help="'utt_id path.npy' lines: one phoneme index per feature frame (use_ph models)")


def load_conditioning(config, utts, utt2spk=None, spk_list=None, ph_scp=None):
    """The tables a conditioned checkpoint needs, checked against the model's configuration and the utterance list without touching the
    GPU: a ``Conditioning`` (articulatory_amd/bin/train.py), or None for an unconditioned model."""
    gp = config.get("generator_params", {})
    use_spk, use_ph = bool(gp.get("use_spk_id", False)), bool(gp.get("use_ph", False))
    if use_spk and not utt2spk:
        raise ValueError("the checkpoint is speaker-conditioned (use_spk_id): --utt2spk is required")
    if use_ph and not ph_scp:
        raise ValueError("the checkpoint is phoneme-conditioned (use_ph): --ph-scp is required")
    if (utt2spk or spk_list) and not use_spk:
        raise ValueError("--utt2spk / --spk-list given, but the checkpoint is not speaker-conditioned (use_spk_id)")
    if ph_scp and not use_ph:
        raise ValueError("--ph-scp given, but the checkpoint is not phoneme-conditioned (use_ph)")
    if not (use_spk or use_ph):
        return None
    from articulatory_amd.bin.train import Conditioning

    spks = None
    if spk_list:
        with open(spk_list) as f:
            spks = [line.strip() for line in f if line.strip()]
    cond = Conditioning(utt2spk=utt2spk, ph_scp=ph_scp, spks=spks)
    if use_spk and len(cond.spks) > int(gp["num_spk"]):
        raise ValueError(f"{len(cond.spks)} speakers for a model with num_spk={gp['num_spk']}: pass the training set's --spk-list")
    for utt in utts:
        if use_spk and utt not in cond.utt2spk:
            raise ValueError(f"utterance {utt!r} is missing from --utt2spk")
        if use_ph and utt not in cond.ph:
            raise ValueError(f"utterance {utt!r} is missing from --ph-scp")
    return cond


def utterance_conditioning(cond, utt_id, frames):
    """(spk_id or None, (frames,) phoneme indices or None) of one utterance."""
    if cond is None:
        return None, None
    e = cond.extras(utt_id, frames)
    ph = e.get("ph")
    if ph is not None and len(ph) != frames:
        raise ValueError(f"utterance {utt_id!r}: {len(ph)} phoneme indices for {frames} frames")
    return e.get("spk_id"), (None if ph is None else torch.as_tensor(np.asarray(ph, dtype=np.int64)))


def get_parser():
    parser = argparse.ArgumentParser(description="Decode dumped features with trained generator.")
    parser.add_argument("--feats-scp", "--scp", default=None, type=str,
                        help="kaldi-style feats.scp file. you need to specify either feats-scp or dumpdir.")
    parser.add_argument("--dumpdir", default=None, type=str,
                        help="directory including feature files. you need to specify either feats-scp or dumpdir.")
    parser.add_argument("--outdir", type=str, required=True, help="directory to save generated speech.")
    parser.add_argument("--checkpoint", type=str, required=True, help="checkpoint file to be loaded.")
    parser.add_argument("--config", default=None, type=str,
                        help="yaml format configuration file. if not explicitly provided, "
                             "it will be searched in the checkpoint directory. (default=None)")
    parser.add_argument("--normalize-before", default=False, action="store_true",
                        help="whether to perform feature normalization before input to the model.")
    parser.add_argument("--verbose", type=int, default=1, help="logging level. higher is more logging. (default=1)")
    parser.add_argument("--batch-size", type=int, default=1,
                        help="utterances synthesised per device call (any lengths; not in the reference, which is batch-1)")
    parser.add_argument("--precision", default=None, choices=("f32", "bf16x3", "bf16x3a"),
                        help="arithmetic of the model's GEMMs, for models with set_precision (the Transformer): f32, the reference's IEEE fp32 "
                             "products, or the opt-in fast modes bf16x3 and (the Transformer only) bf16x3a, which runs the attention on bf16 MFMAs too.  Not given: the model's own default, f32 (not in the reference)")
    parser.add_argument("--dry-run", default=False, action="store_true",
                        help="print this rank's share of the utterance list as one JSON line and exit (no GPU needed; not in the reference)")
    add_conditioning_arguments(parser)
    return parser


def decode_dataset(model, items, config, device, outdir, normalize_before=False, writer=None, batch_size=1, cond=None):
    """The generation loop of decode.py:292-351 for the a2w modes.  Returns (n_utterances, average RTF).
    ``batch_size`` > 1: ragged batches of utterances per device call (RTF = batch time / batch audio).
    ``cond``: the ``Conditioning`` of a speaker- / phoneme-conditioned model (``load_conditioning``)."""
    from articulatory_amd.bin.predict_wav import write_wav

    writer = writer or write_wav
    use_ar = bool(config["generator_params"].get("use_ar", False))
    do_wsola = bool(config.get("wsola", False))
    total_rtf, n = 0.0, 0
    has_spk = cond is not None and cond.utt2spk is not None
    has_ph = cond is not None and cond.ph is not None

    def batch_cond(batch):
        """(list of speaker indices or None, list of phoneme rows or None) of a batch of (utt_id, features)."""
        pairs = [utterance_conditioning(cond, u, int(c.shape[0])) for u, c in batch]
        return [p[0] for p in pairs] if has_spk else None, [p[1] for p in pairs] if has_ph else None

    def forward_cond(spks, phs, lens):
        kw = {}
        if spks is not None:
            kw["spk_id"] = _spk_tensor(spks, device)
        if phs is not None:
            kw["ph"] = _ph_tensor(phs, lens, device)
        return kw

    if batch_size > 1 and not do_wsola:
        with torch.no_grad():
            feats = ((u, torch.tensor(c, dtype=torch.float).to(device)) for u, c in items)
            # AR: a window of 8 batches per device call, continuously batched; non-AR: rectangular-ish batches
            for batch in (windows(feats, 8 * batch_size) if use_ar else length_batches(feats, batch_size)):
                start = time.time()
                xs = [c for _, c in batch]
                spks, phs = batch_cond(batch)
                if use_ar:
                    ys = ar_loop_ragged(model, xs, config, batch=batch_size, spk_id=spks, ph=phs)
                else:
                    if normalize_before:
                        xs = [(c - model.mean) / model.scale for c in xs]
                    padded, lens = pad_utterances(xs)
                    yb = model(padded.permute(0, 2, 1), lengths=lens, **forward_cond(spks, phs, lens))
                    yb = yb[0] if isinstance(yb, tuple) else yb  # (use_ph_loss: (out, ph_out))
                    hop = yb.shape[2] // padded.shape[1]
                    ys = [yb[i, 0, :hop * m] for i, m in enumerate(lens)]
                ys = [y.cpu().numpy() for y in ys]  # device -> host: the synchronisation point the RTF needs
                rtf = (time.time() - start) / (sum(len(y) for y in ys) / config["sampling_rate"])
                for (utt_id, _), y in zip(batch, ys):
                    writer(os.path.join(outdir, f"{utt_id}_gen.wav"), y, config["sampling_rate"])
                    total_rtf += rtf
                    n += 1
        return n, (total_rtf / n if n else float("nan"))
    with torch.no_grad():
        for utt_id, c in items:
            c = torch.tensor(c, dtype=torch.float).to(device)
            start = time.time()
            spk, ph = utterance_conditioning(cond, utt_id, int(c.shape[0]))
            if use_ar:
                y = ar_loop(model, c, config, do_wsola=do_wsola, spk_id=spk, ph=ph)
            elif cond is not None:  # inference() has no way to say who speaks (hifigan.py:298-314): the forward it wraps
                x = (c - model.mean) / model.scale if normalize_before else c
                y = model(x.transpose(1, 0).unsqueeze(0), **forward_cond(None if spk is None else [spk], None if ph is None else [ph],
                                                                       [int(c.shape[0])]))
                y = (y[0] if isinstance(y, tuple) else y).view(-1)
            else:
                y = model.inference(c, normalize_before=normalize_before).view(-1)
            if not do_wsola:
                y = y.cpu().numpy()  # device -> host: also the synchronisation point the RTF needs
                rtf = (time.time() - start) / (len(y) / config["sampling_rate"])
                total_rtf += rtf
                writer(os.path.join(outdir, f"{utt_id}_gen.wav"), y, config["sampling_rate"])
            else:
                signals, arts = y
                for cyi, cy in enumerate(signals):
                    cy = cy.cpu().numpy()
                    rtf = (time.time() - start) / (len(cy) / config["sampling_rate"])
                    total_rtf += rtf
                    writer(os.path.join(outdir, "%s_%d_gen.wav" % (utt_id, cyi)), cy, config["sampling_rate"])
                    np.save(os.path.join(outdir, "%s_%d.npy" % (utt_id, cyi)), arts[cyi].cpu().numpy())
            n += 1
    return n, (total_rtf / n if n else float("nan"))


def decode_features(model, items, config, device, outdir, normalize_before=False, batch_size=1):
    """The generation loop of decode.py:292-351 for the feature-to-feature modes (``art``, ``a2m``) of a non-AR model:
    ``model.inference(c, normalize_before=...)`` saved as ``<utt_id>_gen.npy`` with shape (T, out_channels) (decode.py:348-350).
    ``batch_size`` > 1: ragged batches of similar lengths through ``model(..., lengths=)``, every utterance computed as if alone.
    Returns (n_utterances, average seconds per utterance)."""
    total, n = 0.0, 0
    with torch.no_grad():
        if batch_size > 1:
            feats = ((u, torch.tensor(c, dtype=torch.float).to(device)) for u, c in items)
            for batch in length_batches(feats, batch_size):
                start = time.time()
                xs = [(c - model.mean) / model.scale if normalize_before else c for _, c in batch]
                padded, lens = pad_utterances(xs)
                yb = model(padded.permute(0, 2, 1), lengths=lens)  # (B, out_channels, T_max)
                ys = [yb[i, :, :m].transpose(0, 1).cpu().numpy() for i, m in enumerate(lens)]  # device -> host: the synchronisation point
                total += time.time() - start
                for (utt_id, _), y in zip(batch, ys):
                    np.save(os.path.join(outdir, f"{utt_id}_gen.npy"), y)
                    n += 1
        else:
            for utt_id, c in items:
                c = torch.tensor(c, dtype=torch.float).to(device)
                start = time.time()
                y = model.inference(c, normalize_before=normalize_before).cpu().numpy()
                total += time.time() - start
                np.save(os.path.join(outdir, f"{utt_id}_gen.npy"), y)
                n += 1
    return n, (total / n if n else float("nan"))


def main(argv=None):
    from articulatory_amd.utils import load_model

    args = get_parser().parse_args(argv)
    level = logging.DEBUG if args.verbose > 1 else logging.INFO if args.verbose > 0 else logging.WARN
    logging.basicConfig(level=level, format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s")
    if args.verbose <= 0:
        logging.warning("Skip DEBUG/INFO messages")
    if not os.path.exists(args.outdir):
        os.makedirs(args.outdir)
    if args.config is None:
        args.config = os.path.join(os.path.dirname(args.checkpoint), "config.yml")
    with open(args.config) as f:
        config = yaml.load(f, Loader=yaml.Loader)
    config.update(vars(args))
    if (args.feats_scp is not None and args.dumpdir is not None) or (args.feats_scp is None and args.dumpdir is None):
        raise ValueError("Please specify either --dumpdir or --feats-scp.")
    dataset_mode = config.setdefault("dataset_mode", "default")
    if dataset_mode not in _A2W_MODES + _FEAT_MODES:
        raise NotImplementedError(f"dataset_mode {dataset_mode!r}: only the articulatory/mel -> waveform modes {_A2W_MODES} and the "
                                  f"feature -> feature modes {_FEAT_MODES} are built (SURVEY.md §8 f3)")
    if dataset_mode in _FEAT_MODES and config.get("generator_params", {}).get("use_ar", False):
        raise NotImplementedError(f"dataset_mode {dataset_mode!r} with use_ar: ar_loop's feature branches are not built")
    if config.get("transform") or config.get("input_transform"):
        raise NotImplementedError("feature transforms are not built")
    pairs = list_features(args.feats_scp, args.dumpdir, config.get("format", "npy"))
    logging.info(f"The number of features to be decoded = {len(pairs)}.")
    # a conditioned checkpoint: its tables are read and checked against the whole list here, before any GPU is touched
    cond = load_conditioning(config, [u for u, _ in pairs], args.utt2spk, args.spk_list, args.ph_scp)

    # under torchrun (one process per GPU) every rank decodes its own share of the list and writes its own files
    from articulatory_amd.bin.shard import shard_items
    # shard the (utt_id, path) list first — lengths from the .npy headers — and load each rank's utterances lazily, one at a
    # time (every rank loading the whole dataset would cost N x the I/O and a full copy in host RAM per rank)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        pairs = shard_items(pairs, length_of=lambda kv: npy_frames(kv[1]))
    if args.dry_run:  # what this rank would decode, without touching a GPU (tests/test_distributed_gloo.py runs it under an 8-rank torchrun)
        import json
        print(json.dumps({"rank": int(os.environ.get("RANK", "0")), "world_size": int(os.environ.get("WORLD_SIZE", "1")),
                          "local_rank": int(os.environ.get("LOCAL_RANK", "0")), "utterances": [u for u, _ in pairs],
                          "frames": int(sum(npy_frames(pth) for _, pth in pairs))}), flush=True)
        return
    if not torch.cuda.is_available():
        raise RuntimeError("decode: no GPU visible; this package has no CPU synthesis path")
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    items = load_features(pairs)
    device = torch.device("cuda")
    model = load_model(args.checkpoint, config)
    logging.info(f"Loaded model parameters from {args.checkpoint}.")
    if args.normalize_before:
        assert hasattr(model, "mean"), "Feature stats are not registered."
        assert hasattr(model, "scale"), "Feature stats are not registered."
    model.remove_weight_norm()
    if args.precision is not None:
        if hasattr(model, "set_precision"):
            model.set_precision(args.precision)  # (a class with one arithmetic refuses the other with its own message)
        elif args.precision != "f32":
            raise NotImplementedError(f"--precision {args.precision}: {type(model).__name__} runs in the exact-fp32 arithmetic only")
    model = model.eval().to(device)
    print(sum(p.numel() for p in model.parameters() if p.requires_grad))
    if dataset_mode in _FEAT_MODES:
        n, sec = decode_features(model, items, config, device, config["outdir"], normalize_before=args.normalize_before,
                                 batch_size=args.batch_size)
        logging.info(f"Finished generation of {n} utterances ({sec:.03f} s per utterance).")
        return
    n, rtf = decode_dataset(model, items, config, device, config["outdir"], normalize_before=args.normalize_before,
                            batch_size=args.batch_size, cond=cond)
    logging.info(f"Finished generation of {n} utterances (RTF = {rtf:.03f}).")


if __name__ == "__main__":
    main()
