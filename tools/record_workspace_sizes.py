#!/usr/bin/env python
"""Records the value of every size query of include/hificar.h over a small shape table -> tests/golden/workspace_sizes.json.

The file pins the carving of every workspace, tape and training workspace: tests/test_workspace_sizes_host.py asks the library in the
tree the same questions and expects the same numbers.  It is recorded from the library of the commit BEFORE a change to the planners
(HIFICAR_LIB=<that build's libhificar.so>, or a checkout of that commit), never from the code under test.

    python tools/record_workspace_sizes.py --commit <hash>            the "host" section: queries that answer without a device
    python tools/record_workspace_sizes.py --commit <hash> --device   ... and the "device" section: queries that answer 0 before finalize,
                                                                      the training state or a device-side create (needs the GPU)

Each section maps "<handle>|<query>|<arguments>" to the number the query returned.  cases(lib, device) below is the one place the handles,
shapes and queries are written down; the test walks the same generator.
"""

import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from articulatory_amd import _native  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "workspace_sizes.json")

BATCHES = (1, 2, 3, 64)
FRAMES = (1, 2, 255, 256, 257, 300)            # T, Tl, L or Mp, as the query takes it: both sides of a 256-row tile and of a 32-frame bucket
PACKED_ROWS = FRAMES + (512, 768)              # Mp: whole granules of 256 rows are the only sizes that answer
SAMPLES = (400, 401, 719, 720, 16000, 160000)  # HuBERT's L: the first frame, the second frame, one and ten seconds
FACTORS = (1, 2, 4, 16)

# generator_params of the reference's e2w_hifigan.yaml (tests/conftest.py: E2W_PARAMS), with 2, 3 and 4 residual blocks per stage
GEN = dict(in_channels=141, out_channels=1, channels=512, kernel_size=7, upsample_scales=[5, 4, 2, 2], upsample_kernel_sizes=[10, 8, 4, 4],
           resblock_kernel_sizes=[3, 7, 11], resblock_dilations=[[1, 3, 5]] * 3, use_additional_convs=True, bias=True,
           nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.1}, use_weight_norm=True, use_tanh=True, use_ar=True,
           ar_input=512, ar_hidden=256, ar_output=128)
GEN_BLOCKS = {2: [3, 7], 3: [3, 7, 11], 4: [3, 5, 7, 11]}
GBLOCK = dict(in_channels=141, out_channels=1, channels=64, kernel_size=7, g_scales=[5, 1, 4, 1, 1, 2, 1, 2, 1, 1], g_kernel_sizes=[3] * 10,
              use_weight_norm=True, use_ar=True, ar_input=512, ar_hidden=256, ar_output=128, use_tanh=True)
BIGRU = dict(in_channels=13, hidden_size=64, out_channels=12, use_tanh=False)
XFMR = dict(in_channels=13, out_channels=12, elayers=1, hidden_dim=128)
HUBERT = dict(conv_dim=[64] * 7, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2)
WAVLM_TABLE = dict(num_buckets=8, max_bucket_distance=16)
XFMR_EVAL = ("F32", "BF16X3", "BF16X3A")
XFMR_TRAIN = ("F32", "BF16X3", "BF16X3W", "BF16X3WA", "BF16X3WAC", "BF16X3WACK")
HUBERT_EVAL = ("F32", "BF16X3", "BF16X3A")


class _Handle:
    """One native handle: created by ``hificar_<kind>_create``-style ``create(byref(handle))``, destroyed at the end of its block."""

    def __init__(self, lib, destroy, create):
        self.lib, self.destroy, self.h = lib, destroy, ctypes.c_void_p()
        _native.check(create(ctypes.byref(self.h)), destroy.replace("destroy", "create"))

    def __enter__(self):
        return self.h

    def __exit__(self, *exc):
        getattr(self.lib, self.destroy)(self.h)


def _load(lib, prefix, handle, state, finalize=True):
    """set_weight of every tensor of ``state`` ({name: numpy fp32}), then finalize (the device)."""
    for name, v in state.items():
        if name in ("mean", "scale") or name.endswith("num_batches_tracked"):  # (as NativeFeatureModel.native_state)
            continue
        v = np.ascontiguousarray(v, dtype=np.float32)
        shape = (ctypes.c_int64 * v.ndim)(*v.shape)
        _native.check(getattr(lib, prefix + "_set_weight")(handle, name.encode(), v.ctypes.data_as(ctypes.c_void_p), shape, v.ndim), prefix + "_set_weight")
    if finalize:
        _native.check(getattr(lib, prefix + "_finalize")(handle), prefix + "_finalize")


def _generator_cases(lib, device):
    if device:
        return
    for nb, ks in GEN_BLOCKS.items():
        params = dict(GEN, resblock_kernel_sizes=ks, resblock_dilations=[[1, 3, 5]] * nb)
        cfg = _native.make_config(params, _native.PREC_F32)
        with _Handle(lib, "hificar_destroy", lambda out: lib.hificar_create(ctypes.byref(cfg), out)) as h:
            for prec in ("F32", "BF16X3"):
                _native.check(lib.hificar_set_precision(h, _native.CONSTANTS["PREC_" + prec]), "hificar_set_precision")
                for q in ("hificar_workspace_bytes", "hificar_tape_bytes", "hificar_backward_workspace_bytes"):
                    for B in BATCHES:
                        for T in FRAMES:
                            yield f"generator.blocks{nb}.{prec}|{q}|B={B},T={T}", getattr(lib, q)(h, B, T)
    cfg = _native.make_gblock_config(GBLOCK, _native.PREC_F32)
    with _Handle(lib, "hificar_destroy", lambda out: lib.hificar_gblock_create(ctypes.byref(cfg), out)) as h:
        for q in ("hificar_workspace_bytes", "hificar_tape_bytes", "hificar_backward_workspace_bytes"):
            for B in BATCHES:
                for T in FRAMES:
                    yield f"gblock|{q}|B={B},T={T}", getattr(lib, q)(h, B, T)


def _disc_mel_cases(lib, device):
    """The discriminators and the mel / STFT losses: their create calls set device state up, so every query of theirs is a device query."""
    if not device:
        return
    from articulatory_amd.models.discriminator import HiFiGANMultiScaleMultiPeriodDiscriminator

    cfg = HiFiGANMultiScaleMultiPeriodDiscriminator()._config()
    with _Handle(lib, "hificar_disc_destroy", lambda out: lib.hificar_disc_create(ctypes.byref(cfg), out)) as h:
        for q in ("hificar_disc_tape_bytes", "hificar_disc_backward_workspace_bytes", "hificar_disc_dout_floats"):
            for B in BATCHES:
                for T in FRAMES:
                    yield f"disc|{q}|B={B},T={T}", getattr(lib, q)(h, B, T)
    melmat = np.ones((80, 513), dtype=np.float32)
    for mode, mcfg in (("mel", _native.HificarMelConfig(1024, 256, 1024, 80, 1e-10, 10, 0)), ("stft", _native.HificarMelConfig(1024, 120, 600, 0, 1e-7, 0, 1))):
        with _Handle(lib, "hificar_mel_destroy", lambda out: lib.hificar_mel_create(ctypes.byref(mcfg), melmat.ctypes.data_as(ctypes.c_void_p), out)) as h:
            for B in BATCHES:
                for T in FRAMES + (8192,):
                    yield f"{mode}|hificar_mel_workspace_bytes|B={B},T={T}", lib.hificar_mel_workspace_bytes(h, B, T)


def _feat_cases(lib, device):
    if device:
        return
    melmat = np.ones((40, 161), dtype=np.float32)
    for kind, cfg in (("mfcc", _native.HificarFeatConfig(_native.FEAT_MFCC, 320, 160, 320, 40, 13, 1e-10, 80.0, 10)),
                      ("logmel", _native.HificarFeatConfig(_native.FEAT_LOGMEL, 320, 160, 320, 40, 0, 1e-10, 80.0, 10))):
        with _Handle(lib, "hificar_feat_destroy", lambda out: lib.hificar_feat_create(ctypes.byref(cfg), melmat.ctypes.data_as(ctypes.c_void_p), out)) as h:
            for B in BATCHES:
                for L in FRAMES + SAMPLES:
                    yield f"feat.{kind}|hificar_feat_workspace_bytes|B={B},L={L}", lib.hificar_feat_workspace_bytes(h, B, L)


def _bigru_cases(lib, device):
    from articulatory_amd.utils.synth import synth_bigru_state_dict

    cfg = _native.make_bigru_config(BIGRU)
    with _Handle(lib, "hificar_bigru_destroy", lambda out: lib.hificar_bigru_create(ctypes.byref(cfg), out)) as h:
        if device:
            _load(lib, "hificar_bigru", h, synth_bigru_state_dict(BIGRU, seed=1))
        plain = ("hificar_bigru_train_workspace_bytes",) if device else ("hificar_bigru_workspace_bytes", "hificar_bigru_tape_bytes")
        low = ("hificar_bigru_train_workspace_bytes_lowrate",) if device else ("hificar_bigru_workspace_bytes_lowrate", "hificar_bigru_tape_bytes_lowrate")
        for B in BATCHES:
            for T in FRAMES:
                for q in plain:
                    yield f"bigru|{q}|B={B},T={T}", getattr(lib, q)(h, B, T)
                for f in FACTORS:
                    for q in low:
                        yield f"bigru|{q}|B={B},Tl={T},factor={f}", getattr(lib, q)(h, B, T, f)


def _xfmr_cases(lib, device):
    from articulatory_amd.utils.synth import synth_transformer_state_dict

    cfg = _native.make_xfmr_config(XFMR)
    for prec in XFMR_EVAL:
        if device and prec != "F32":  # (a handle packed for another inference arithmetic has no training step)
            continue
        with _Handle(lib, "hificar_xfmr_destroy", lambda out: lib.hificar_xfmr_create(ctypes.byref(cfg), out)) as h:
            _native.check(lib.hificar_xfmr_set_precision(h, _native.CONSTANTS["PREC_" + prec]), "hificar_xfmr_set_precision")
            if not device:
                for B in BATCHES:
                    for T in FRAMES:
                        yield f"xfmr.{prec}|hificar_xfmr_workspace_bytes|B={B},T={T}", lib.hificar_xfmr_workspace_bytes(h, B, T)
                        for f in FACTORS:
                            yield f"xfmr.{prec}|hificar_xfmr_workspace_bytes_lowrate|B={B},Tl={T},factor={f}", lib.hificar_xfmr_workspace_bytes_lowrate(h, B, T, f)
                continue
            _load(lib, "hificar_xfmr", h, synth_transformer_state_dict(XFMR, seed=1))
            for tp in XFMR_TRAIN:
                _native.check(lib.hificar_xfmr_set_train_precision(h, _native.CONSTANTS["PREC_" + tp]), "hificar_xfmr_set_train_precision")
                for B in BATCHES:
                    for T in FRAMES:
                        for q in ("hificar_xfmr_tape_bytes", "hificar_xfmr_train_workspace_bytes"):
                            yield f"xfmr.train.{tp}|{q}|B={B},T={T}", getattr(lib, q)(h, B, T)
                    for Mp in PACKED_ROWS:
                        for q in ("hificar_xfmr_tape_bytes_packed", "hificar_xfmr_train_workspace_bytes_packed"):
                            yield f"xfmr.train.{tp}|{q}|B={B},Mp={Mp}", getattr(lib, q)(h, B, Mp)


def _hubert_cases(lib, device):
    if device:
        return
    config = _native.check_hubert_config(HUBERT)
    cfg = _native.make_hubert_config(config, True, 1e-7)
    for prec in HUBERT_EVAL:
        for rel in (False, True):
            if rel and prec == "BF16X3A":  # (the bf16 attention kernel has no bias term: refused)
                continue
            with _Handle(lib, "hificar_hubert_destroy", lambda out: lib.hificar_hubert_create(ctypes.byref(cfg), out)) as h:
                _native.check(lib.hificar_hubert_set_precision(h, _native.CONSTANTS["PREC_" + prec]), "hificar_hubert_set_precision")
                if rel:
                    nb, md = WAVLM_TABLE["num_buckets"], WAVLM_TABLE["max_bucket_distance"]
                    table = _native.wavlm_bucket_of_distance(nb, md)
                    _native.check(lib.hificar_hubert_set_rel_bias(h, nb, md, ctypes.c_void_p(table.data_ptr())), "hificar_hubert_set_rel_bias")
                for sub in (0, 1):
                    _native.check(lib.hificar_hubert_debug_sub_batch(h, sub), "hificar_hubert_debug_sub_batch")
                    for B in BATCHES:
                        for L in SAMPLES:
                            yield (f"hubert.{prec}.{'rel_bias' if rel else 'plain'}.sub{sub}|hificar_hubert_workspace_bytes|B={B},L={L}",
                                   lib.hificar_hubert_workspace_bytes(h, B, L))


def _linear_cases(lib, device):
    """hificar_linear_create uploads the map: a device query."""
    if not device:
        return
    import torch

    coef, intercept = torch.zeros(12, 1024), torch.zeros(12)
    with _Handle(lib, "hificar_linear_destroy", lambda out: lib.hificar_linear_create(1024, 12, coef.data_ptr(), intercept.data_ptr(), out)) as h:
        for B in BATCHES:
            for T in FRAMES:
                yield f"linear|hificar_linear_workspace_bytes|B={B},T={T}", lib.hificar_linear_workspace_bytes(h, B, T)


def cases(lib, device):
    """(key, value) of every query of one section, from ``lib``: device False -> "host" (no device is touched), True -> "device"."""
    for part in (_generator_cases, _disc_mel_cases, _feat_cases, _bigru_cases, _xfmr_cases, _hubert_cases, _linear_cases):
        for key, value in part(lib, device):
            yield key, int(value)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", required=True, help="the commit the loaded library was built from (written into the file)")
    ap.add_argument("--device", action="store_true", help="also record the device section (needs the GPU)")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    lib = _native.load_library()
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc["commit"] = args.commit
    doc["host"] = dict(cases(lib, False))
    if args.device:
        doc["device"] = dict(cases(lib, True))
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: host {len(doc['host'])} queries, device {len(doc.get('device', {}))} queries, commit {doc['commit']}")


if __name__ == "__main__":
    main()
