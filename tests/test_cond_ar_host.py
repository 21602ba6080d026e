"""Conditioned AR synthesis, the parts that need no GPU: the oracle against the reference's chunked loop of a speaker- / phoneme-
conditioned generator (tests/golden/gold_arloop_cond.npz, tools/make_golden_arloop_cond.py), the host-side checks of the three
``*_cond`` C entry points (hificar_ar_loop_cond, hificar_ar_loop_packed_cond, hificar_ar_step_cond) on a handle that is never
finalized, and the refusals of the Python layer and the command lines that are decided before a device is asked for."""

import ctypes
import json
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import E2W_PARAMS, GOLDEN, rel_err
from articulatory_amd import _native
from articulatory_amd.bin import decode, predict_wav
from articulatory_amd.models import HiFiGANGenerator
from articulatory_amd.streaming import StreamingSynthesizer
from articulatory_amd.utils.synth import synth_state_dict
from oracle import hificar_oracle as O

SPK_PARAMS = dict(E2W_PARAMS, channels=128, use_spk_id=True, num_spk=5, spk_emb_size=32)
PH_PARAMS = dict(E2W_PARAMS, channels=128, in_channels=13 + 128 + 8, use_ph=True, num_ph=11, ph_emb_size=8)
CASES = {"spk": (SPK_PARAMS, 4321), "ph": (PH_PARAMS, 4323)}


def oracle_loop(w, params, x, chunk, spk=None, ph=None):
    """The definition: chunks of `chunk` frames (the last one shorter), prev = zeros, then the last ar_input samples of the previous
    chunk's output, every chunk through the oracle's forward with the utterance's speaker and the chunk's slice of its phoneme row."""
    prev = torch.zeros((1, 1, params["ar_input"]))
    outs = []
    for i in range(0, len(x), chunk):
        y = O.generator_forward(w, params, x[i:i + chunk].t()[None], prev, spk_id=None if spk is None else torch.tensor([spk]),
                                ph=None if ph is None else ph[None, i:i + chunk])
        outs.append(y[0, 0])
        prev = y[:, :, -params["ar_input"]:]
    return torch.cat(outs)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_oracle_loop_reproduces_the_reference(tag):
    gold = np.load(os.path.join(GOLDEN, "gold_arloop_cond.npz"))
    params, seed = CASES[tag]
    w = O.fold_weight_norm(synth_state_dict(params, seed=seed))
    chunk = int(gold["chunk_frames"])
    assert chunk == 25 and [int(v) for v in gold["lengths"]] == [60, 260]
    for T in (60, 260):
        x = torch.from_numpy(gold[f"{tag}_x{T}"])
        spk = int(gold[f"spk_spk{T}"]) if tag == "spk" else None
        ph = torch.from_numpy(gold[f"ph_ph{T}"]) if tag == "ph" else None
        with torch.no_grad():
            y = oracle_loop(w, params, x, chunk, spk, ph)
        assert y.shape == (80 * T,)
        err = rel_err(y.numpy(), gold[f"{tag}_out{T}"])
        print(f"{tag} T={T}: oracle vs reference {err:.3e}")
        assert err < 2e-6, (tag, T)
        assert float(gold[f"{tag}_f32_dev{T}"]) < 1e-5  # the reference's own fp32-vs-fp64 deviation: the loop is well conditioned


# ---- C ABI: host-side checks on an un-finalized handle (nothing is ever enqueued, no pointer dereferenced) --------------------------
@pytest.fixture(scope="module")
def lib():
    return _native.load_library()


def _handle(lib, **over):
    p = dict(E2W_PARAMS, use_tanh=True)
    p.update(over)
    cfg = _native.make_config(p, _native.PREC_F32)
    h = ctypes.c_void_p()
    assert lib.hificar_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, lib.hificar_last_error()
    return h


DUMMY = ctypes.c_void_p(256)
SPK = dict(use_spk_id=True, num_spk=4, spk_emb_size=8)
PH = dict(use_ph=True, num_ph=11, ph_emb_size=8, in_channels=141 + 8)


def _loop(lib, h, spk, ph):
    rc = lib.hificar_ar_loop_cond(h, DUMMY, spk, ph, None, None, DUMMY, 2, 60, 25, DUMMY, 1 << 30, None)
    return rc, lib.hificar_last_error().decode()


def _packed(lib, h, spk, ph):
    lens = np.array([60, 30], dtype=np.int32)
    rc = lib.hificar_ar_loop_packed_cond(h, DUMMY, spk, ph, lens.ctypes.data_as(ctypes.c_void_p), DUMMY, 2, 60, 25, 2, DUMMY, 1 << 30, None)
    return rc, lib.hificar_last_error().decode()


def _step(lib, h, spk, ph, table, ph_bstride=100, chunk=25, ctx_rows=4, c_cstride=100):
    t = np.ascontiguousarray(table, dtype=np.int32).reshape(-1, 4)
    rc = lib.hificar_ar_step_cond(h, DUMMY, 13 * c_cstride, c_cstride, spk, ph, ph_bstride, t.ctypes.data_as(ctypes.c_void_p), t.shape[0],
                                  chunk, DUMMY, ctx_rows, DUMMY, DUMMY, 1 << 30, None)
    return rc, lib.hificar_last_error().decode()


GOOD_TABLE = [[0, 0, 25, 1], [3, 50, 10, 0]]


def test_cabi_symbols_exist(lib):
    for name in ("hificar_ar_loop_cond", "hificar_ar_loop_packed_cond", "hificar_ar_step_cond"):
        assert name in _native.SYMBOLS
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("over,have,missing", [(SPK, "spk", "spk_id"), (PH, "ph", "ph")])
def test_cabi_missing_and_superfluous_conditioning(lib, over, have, missing):
    h = _handle(lib, **over)
    good = dict(spk=DUMMY if have == "spk" else None, ph=DUMMY if have == "ph" else None)
    other = dict(spk=DUMMY, ph=DUMMY)
    try:
        for call in (_loop, _packed, lambda lb, hh, spk, ph: _step(lb, hh, spk, ph, GOOD_TABLE)):
            rc, msg = call(lib, h, None, None)
            assert rc == -1 and f"needs {missing}" in msg, msg
            rc, msg = call(lib, h, other["spk"], other["ph"])
            assert rc == -1 and "given to a model built with" in msg, msg
            rc, msg = call(lib, h, good["spk"], good["ph"])  # well formed: reaches the state check
            assert rc == -2 and "finalize" in msg, msg
    finally:
        lib.hificar_destroy(h)


def test_cabi_plain_model_takes_no_conditioning(lib):
    h = _handle(lib)
    try:
        for call in (_loop, _packed, lambda lb, hh, spk, ph: _step(lb, hh, spk, ph, GOOD_TABLE)):
            rc, msg = call(lib, h, DUMMY, None)
            assert rc == -1 and "use_spk_id=false" in msg, msg
            rc, msg = call(lib, h, None, DUMMY)
            assert rc == -1 and "use_ph=false" in msg, msg
            rc, msg = call(lib, h, None, None)  # null conditioning: the old entry point
            assert rc == -2 and "finalize" in msg, msg
    finally:
        lib.hificar_destroy(h)


def test_cabi_step_table_checks_with_a_phoneme_ring(lib):
    h = _handle(lib, **PH)
    try:
        def err(table, **kw):
            return _step(lib, h, None, DUMMY, table, **kw)

        rc, msg = err([[0, 80, 25, 0]], ph_bstride=100, c_cstride=200)  # fits the feature rows, overruns the phoneme ring
        assert rc == -1 and "phoneme ring" in msg and "[80, 105)" in msg, msg
        rc, msg = err([[0, 75, 25, 0]], ph_bstride=100, c_cstride=200)
        assert rc == -2, msg
        rc, msg = err([[0, 0, 25, 1]], ph_bstride=0)
        assert rc == -1 and "row pitch" in msg, msg
        # every table error of hificar_ar_step
        rc, msg = err([[4, 0, 25, 1]])
        assert rc == -1 and "row 4 outside [0, 4)" in msg
        rc, msg = err([[-1, 0, 25, 1]])
        assert rc == -1 and "outside" in msg
        rc, msg = err([[1, 0, 25, 1], [1, 25, 25, 0]])
        assert rc == -1 and "appears twice" in msg
        rc, msg = err([[0, 0, 0, 1]])
        assert rc == -1 and "valid frames 0 outside [1, 25]" in msg
        rc, msg = err([[0, 0, 26, 1]])
        assert rc == -1 and "valid frames 26" in msg
        rc, msg = err([[0, 90, 25, 1]])
        assert rc == -1 and "feature rows" in msg
        rc, msg = err([[0, 0, 6, 1]], chunk=6)
        assert rc == -1 and "ar_input (512) > chunk audio length (480)" in msg
        rc, msg = err([[0, 0, 25, 1]] * 5, ctx_rows=4)
        assert rc == -1
        assert lib.hificar_ar_step_cond(h, None, 0, 1, None, DUMMY, 100, None, 1, 25, None, 4, None, None, 0, None) == -1
        assert "null argument" in lib.hificar_last_error().decode()
        rc, msg = err(GOOD_TABLE)
        assert rc == -2 and "finalize" in msg
    finally:
        lib.hificar_destroy(h)


@pytest.mark.parametrize("over", [SPK, PH])
def test_cabi_old_entry_points_still_refuse_conditioned_models(lib, over):
    h = _handle(lib, **over)
    t = np.array([[0, 0, 25, 1]], dtype=np.int32)
    lens = np.array([60], dtype=np.int32)
    try:
        assert lib.hificar_ar_loop_ragged(h, DUMMY, None, None, DUMMY, 1, 60, 25, DUMMY, 1 << 30, None) == -1
        assert "conditioned" in lib.hificar_last_error().decode()
        assert lib.hificar_ar_loop(h, DUMMY, DUMMY, 1, 60, 25, DUMMY, 1 << 30, None) == -1
        assert "conditioned" in lib.hificar_last_error().decode()
        assert lib.hificar_ar_loop_packed(h, DUMMY, lens.ctypes.data_as(ctypes.c_void_p), DUMMY, 1, 60, 25, 1, DUMMY, 1 << 30, None) == -1
        assert "conditioned" in lib.hificar_last_error().decode()
        assert lib.hificar_ar_step(h, DUMMY, 1300, 100, t.ctypes.data_as(ctypes.c_void_p), 1, 25, DUMMY, 4, DUMMY, DUMMY, 1 << 30, None) == -1
        assert "conditioned" in lib.hificar_last_error().decode()
    finally:
        lib.hificar_destroy(h)


# ---- Python refusals that need no device -------------------------------------------------------------------------------------------
class _NoHandle:
    """Fails the test if the constructor gets as far as asking for the native handle."""

    def __init__(self, model):
        self.__dict__["_m"] = model

    def __getattr__(self, name):
        if name == "_native_handle":
            raise AssertionError("the handle was asked for before the refusal")
        return getattr(self._m, name)


def test_streaming_opt_in_is_explicit_both_ways():
    plain = HiFiGANGenerator(**E2W_PARAMS)
    with pytest.raises(ValueError, match="conditioned=True needs"):
        StreamingSynthesizer(_NoHandle(plain), 25, conditioned=True)
    for over in (SPK, PH):
        cond = HiFiGANGenerator(**dict(E2W_PARAMS, **over))
        with pytest.raises(ValueError, match="conditioned"):
            StreamingSynthesizer(_NoHandle(cond), 25)
        with pytest.raises(RuntimeError, match="no CPU fallback"):  # opted in: gets as far as the device
            StreamingSynthesizer(cond, 25, conditioned=True)


# ---- command lines -----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def dataset(tmp_path):
    lens = [300, 280, 270]
    scp = tmp_path / "feats.scp"
    with open(scp, "w") as f:
        for i, n in enumerate(lens):
            np.save(tmp_path / f"u{i}.npy", np.zeros((n, 13)))
            np.save(tmp_path / f"u{i}-ph.npy", np.zeros((n,), dtype=np.int64))
            f.write(f"u{i} {tmp_path / f'u{i}.npy'}\n")
    (tmp_path / "utt2spk").write_text("u0 bob\nu1 alice\nu2 bob\n")
    (tmp_path / "utt2spk_short").write_text("u0 bob\nu2 bob\n")
    (tmp_path / "ph.scp").write_text("".join(f"u{i} {tmp_path / f'u{i}-ph.npy'}\n" for i in range(3)))
    (tmp_path / "ph_short.scp").write_text(f"u0 {tmp_path / 'u0-ph.npy'}\n")
    (tmp_path / "spks").write_text("zoe\nbob\nalice\n")

    def config(**gp):
        p = tmp_path / f"config_{'_'.join(sorted(gp)) or 'plain'}.yml"
        p.write_text(yaml.safe_dump({"format": "npy", "generator_type": "HiFiGANGenerator", "batch_max_steps": 2000, "hop_size": 80,
                                     "generator_params": dict(gp)}))
        return str(p)

    def argv(cfg, *more):
        return ["--feats-scp", str(scp), "--outdir", str(tmp_path / "out"), "--checkpoint", str(tmp_path / "ckpt.pkl"), "--config", cfg,
                "--verbose", "0", *more]

    return tmp_path, config, argv


def test_cli_conditioned_checkpoint_needs_its_tables(dataset, monkeypatch):
    tmp, config, argv = dataset
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the GPU was asked for before the refusal"))
    spk_cfg, ph_cfg = config(use_spk_id=True, num_spk=3, spk_emb_size=8), config(use_ph=True, num_ph=11, ph_emb_size=8)
    for main in (decode.main, predict_wav.main):
        with pytest.raises(ValueError, match="--utt2spk"):
            main(argv(spk_cfg))
        with pytest.raises(ValueError, match="--ph-scp"):
            main(argv(ph_cfg))
        with pytest.raises(ValueError, match="'u1' is missing from --utt2spk"):
            main(argv(spk_cfg, "--utt2spk", str(tmp / "utt2spk_short")))
        with pytest.raises(ValueError, match="'u1' is missing from --ph-scp"):
            main(argv(ph_cfg, "--ph-scp", str(tmp / "ph_short.scp")))
        with pytest.raises(ValueError, match="not speaker-conditioned"):
            main(argv(config(), "--utt2spk", str(tmp / "utt2spk")))


def test_cli_dry_run_lists_the_same_utterances(dataset, capsys):
    tmp, config, argv = dataset

    def listed(*a):
        decode.main(argv(*a, "--dry-run"))
        return json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])

    plain = listed(config())
    spk = listed(config(use_spk_id=True, num_spk=3, spk_emb_size=8), "--utt2spk", str(tmp / "utt2spk"), "--spk-list", str(tmp / "spks"))
    ph = listed(config(use_ph=True, num_ph=11, ph_emb_size=8), "--ph-scp", str(tmp / "ph.scp"))
    assert plain["utterances"] == spk["utterances"] == ph["utterances"] == ["u0", "u1", "u2"]
    assert plain["frames"] == spk["frames"] == ph["frames"] == 850


def test_cli_speaker_indices_follow_the_training_sets_list(dataset):
    tmp, _, _ = dataset
    cfg = {"generator_params": dict(use_spk_id=True, num_spk=3, spk_emb_size=8)}
    utts = ["u0", "u1", "u2"]
    cond = decode.load_conditioning(cfg, utts, utt2spk=str(tmp / "utt2spk"))
    assert [decode.utterance_conditioning(cond, u, 10)[0] for u in utts] == [1, 0, 1]  # sorted speakers: alice, bob
    cond = decode.load_conditioning(cfg, utts, utt2spk=str(tmp / "utt2spk"), spk_list=str(tmp / "spks"))
    assert [decode.utterance_conditioning(cond, u, 10)[0] for u in utts] == [1, 2, 1]  # zoe, bob, alice
    with pytest.raises(ValueError, match="num_spk=2"):
        decode.load_conditioning({"generator_params": dict(use_spk_id=True, num_spk=2)}, utts, utt2spk=str(tmp / "utt2spk"),
                                 spk_list=str(tmp / "spks"))
    cfg = {"generator_params": dict(use_ph=True, num_ph=11, ph_emb_size=8)}
    cond = decode.load_conditioning(cfg, utts, ph_scp=str(tmp / "ph.scp"))
    spk, ph = decode.utterance_conditioning(cond, "u1", 280)
    assert spk is None and ph.shape == (280,) and ph.dtype == torch.int64
    with pytest.raises(ValueError, match="'u2': 270 phoneme indices for 300 frames"):
        decode.utterance_conditioning(cond, "u2", 300)
