"""Host-side checks of ragged Transformer training (``pytest -m "not gpu"``): the admission of every shape tests/test_gpu_transformer_ragged.py
runs, the ragged restatement against the dense one and against each sequence alone, the new entry point of the C ABI, and the Python and
trainer surface (``forward_padded``, ``package_mode: pad_masked``).
"""

import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import transformer_ragged_oracle as R
import transformer_train_oracle as O
from conftest import REPO
from articulatory_amd import _native
from articulatory_amd.bin import train as T


@pytest.mark.parametrize("name", list(R.RAGGED_SHAPES))
def test_ragged_shape_is_admitted(name):
    """The admission rule of the dense suite: the restatement's own float32 run is within half of every bar of
    transformer_train_oracle.BARS against its float64 run, and the valid frames are off the L1 kink."""
    ref = R.ragged_restatement(name, torch.float64)
    assert ref["kink"] > O.KINK_MARGIN
    worst = {k: e / bar for k, (e, bar) in O.errors(R.ragged_restatement(name, torch.float32), ref).items()}
    k = max(worst, key=worst.get)
    print(f"{name}: worst fp32 share of a bar: {k} {worst[k]:.3f}")
    assert worst[k] <= 0.5, (k, worst[k])


def test_shapes_are_the_issues_table():
    S = R.RAGGED_SHAPES
    assert list(S) == ["mixed", "tiles", "band", "band2", "zero", "chunks", "d96", "d128", "nores", "b1", "d32", "d64"]
    assert [(v[1], v[2], v[3], v[4]) for v in S.values()] == [
        (3, 70, (70, 33, 1), 0.2), (4, 130, (64, 65, 128, 130), 0.5), (2, 263, (263, 100), 0.2), (2, 201, (201, 99), 0.0),
        (3, 65, (65, 0, 2), 0.0), (3, 200, (200, 57, 143), 0.2), (2, 130, (130, 71), 0.2), (2, 70, (70, 17), 0.2), (2, 65, (65, 40), 0.2),
        (1, 100, (37,), 0.5), (2, 130, (130, 71), 0.2), (2, 130, (130, 71), 0.2)]
    assert S["d96"][0]["hidden_dim"] == 768 and S["d128"][0]["hidden_dim"] == 1024 and S["d96"][0]["elayers"] == S["d128"][0]["elayers"] == 1
    assert S["d32"][0] == dict(S["d96"][0], hidden_dim=256) and S["d64"][0] == dict(S["d96"][0], hidden_dim=512)  # the head sizes people train at
    assert S["nores"][0]["in_channels"] == S["nores"][0]["hidden_dim"] == 128
    assert all(v[0] == O.BASE for k, v in S.items() if k not in ("d96", "d128", "nores", "d32", "d64"))


def test_all_lengths_full_is_the_dense_restatement():
    """The ragged restatement with every length = T against transformer_train_oracle's dense step, in float64: equal to rounding (the
    batch norm sums rows in another order, the loss divides once instead of taking a mean)."""
    params, sd, x, t = O.case("t65")
    B, T = x.shape[0], x.shape[2]
    dense = O.TransformerTrainOracle(sd, dtype=torch.float64, dropout=params["dropout"], seed=O.DROPOUT_SEED)
    ragged = R.TransformerRaggedOracle(sd, dtype=torch.float64, dropout=params["dropout"], seed=O.DROPOUT_SEED)
    a, b = dense.step(x, t), ragged.step_padded(x, t, (T,) * B)
    a["running"], b["running"] = dict(dense.buffers), dict(ragged.buffers)
    for k, (e, _) in O.errors(b, a).items():
        assert e < 1e-11, (k, e)


def test_each_sequence_of_a_ragged_batch_is_that_sequence_alone():
    """At p = 0 the first conv and the attention of a sequence in a ragged batch are those of the sequence alone (float64, to rounding):
    zero padding at its own end, keys below its own length."""
    params, sd, x, _, lengths = R.ragged_case("band2")
    o = R.TransformerRaggedOracle(sd, dtype=torch.float64, dropout=0.0)
    with torch.no_grad():
        c = o.conv1_output(x, lengths)
        rows = torch.from_numpy(np.random.default_rng(3).standard_normal((x.shape[0], x.shape[2], params["hidden_dim"])))
        a = o.attention_output(rows, lengths)
        for b, n in enumerate(lengths):
            alone = o.conv1_output(x[b:b + 1, :, :n], (n,))
            assert float((c[b:b + 1, :, :n] - alone).abs().max()) < 1e-12 and float(c[b, :, n:].abs().max() if n < x.shape[2] else 0.0) == 0.0
            alone = o.attention_output(rows[b:b + 1, :n], (n,))
            assert float((a[b:b + 1, :, :n] - alone).abs().max()) < 1e-12 and float(a[b, :, n:].abs().max() if n < x.shape[2] else 0.0) == 0.0
        # and what the padded frames of x hold does not matter
        dirty = x.copy()
        for b, n in enumerate(lengths):
            dirty[b, :, n:] = np.nan
        assert torch.equal(o.conv1_output(dirty, lengths), c)


def test_three_step_batches_are_admitted():
    """The three `pad_masked` steps of tests/test_gpu_transformer_ragged.py's trainer test: the restatement's own float32 losses within
    half of the device's loss bar of its float64 ones."""
    l32, _ = R.run_steps3(torch.float32)
    l64, _ = R.run_steps3(torch.float64)
    errs = [abs(a - b) / abs(b) for a, b in zip(l32, l64)]
    print("three-step float32 against float64:", errs)
    assert max(errs) <= 0.5 * R.STEPS3_LOSS_BAR
    assert all(max(n) == 70 and len(n) == 3 for n in R.STEPS3_LENGTHS)  # every batch padded to the case's T


def test_ragged_entry_point_in_the_header_and_the_library(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hificar.h"\n'
                   "int use(hificar_xfmr* h, const float* x, float* y, void* p, const int32_t* n) {\n"
                   "    return hificar_xfmr_forward_train_ragged(h, x, n, n, y, y, 2, 5, 0.2f, 1u, 0u, p, hificar_xfmr_tape_bytes(h, 2, 5), p,\n"
                   "                                             hificar_xfmr_train_workspace_bytes(h, 2, 5), 0);\n}\n")
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hificar_xfmr_forward_train_ragged" in _native.SYMBOLS
    lib = _native.load_library()
    assert hasattr(lib, "hificar_xfmr_forward_train_ragged")
    # before finalize: a clean failure that names what is missing (the lengths are not looked at)
    h = ctypes.c_void_p()
    cfg = _native.make_xfmr_config(dict(O.BASE))
    _native.check(lib.hificar_xfmr_create(ctypes.byref(cfg), ctypes.byref(h)), "hificar_xfmr_create")
    try:
        def call(host, B=2, T=5, device=True):
            lens = (ctypes.c_int32 * len(host))(*host) if host is not None else None
            # (the device copy is not read before the handle's state is checked: any non-null pointer stands in for it here)
            return lib.hificar_xfmr_forward_train_ragged(h, None, ctypes.cast(lens, ctypes.c_void_p) if device and host is not None else None,
                                                         ctypes.cast(lens, ctypes.c_void_p) if host is not None else None, None, None, B, T, 0.0, 0, 0,
                                                         None, 0, None, 0, None)

        E_INVALID, E_STATE = -1, -2  # include/hificar.h
        assert call((5, 3)) == E_STATE and b"hificar_xfmr_finalize" in lib.hificar_last_error()
        # the arguments are checked first, before anything is enqueued: a null lengths_host, a length outside 0 .. T, M < 2
        assert call(None) == E_INVALID and b"lengths_host" in lib.hificar_last_error()
        assert call((5, 3), device=False) == E_INVALID and b"lengths_host" in lib.hificar_last_error()
        assert call((5, 6)) == E_INVALID and b"lengths[1]=6 outside [0, 5]" in lib.hificar_last_error()
        assert call((-1, 3)) == E_INVALID and b"lengths[0]=-1" in lib.hificar_last_error()
        assert call((1, 0)) == E_INVALID and b"sum of lengths = 1" in lib.hificar_last_error()
        assert call((0, 0)) == E_INVALID and b"sum of lengths = 0" in lib.hificar_last_error()
        assert call((2, 0)) == E_STATE  # M = 2 with an empty sequence is a batch
    finally:
        lib.hificar_xfmr_destroy(h)


def test_the_header_no_longer_lists_ragged_training_as_not_built():
    text = open(os.path.join(REPO, "include", "hificar.h")).read()
    assert "Not built: ragged Transformer training" not in text
    assert "hificar_xfmr_forward_train_ragged" in text


def config(**kw):
    cfg = dict(generator_type="Transformer", dataset_mode="a2m", generator_params=dict(O.BASE, dropout=0.2), generator_optimizer_type="Adam",
               generator_optimizer_params=dict(lr=1e-3), generator_scheduler_params=dict(step_size=10, gamma=0.5), train_max_steps=100,
               discriminator_train_start_steps=100)
    cfg.update(kw)
    return cfg


def bigru_config(**kw):
    return config(generator_type="BiGRU", dataset_mode="art", generator_params=dict(in_channels=24, hidden_size=64, out_channels=12), **kw)


def test_forward_padded_refuses_before_it_needs_a_device():
    from articulatory_amd.models import Transformer

    m = Transformer(**O.BASE).train()
    with pytest.raises(RuntimeError, match="needs lengths"):
        m.forward_padded(torch.zeros(2, 12, 5), None)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        m.forward_padded(torch.zeros(2, 12, 5), [5, 3])
    with pytest.raises(NotImplementedError, match=r"ragged training.*forward_padded"):  # forward(lengths=) in train() mode points to it
        m(torch.zeros(2, 12, 5), lengths=[5, 3])
    with pytest.raises(RuntimeError, match="CUDA/HIP"):  # eval mode routes to forward(lengths=)
        m.eval().forward_padded(torch.zeros(2, 12, 5), [5, 3])


def test_inversion_trainer_builds_pad_masked_for_both_models():
    cpu = torch.device("cpu")
    tr = T.InversionTrainer(config(package_mode="pad_masked"), cpu)
    from articulatory_amd.models import BiGRU, Transformer

    assert isinstance(tr.G, Transformer) and tr.package_mode == "pad_masked" and tr.padded
    with pytest.raises(ValueError, match="lengths"):
        tr.train_step({"x": torch.zeros(2, 12, 5), "y": torch.zeros(2, 8, 5)})
    # the reference's `pad` stays refused for the Transformer, and the refusal names the way in
    with pytest.raises(NotImplementedError, match=r"package_mode pad .*pad_masked"):
        T.InversionTrainer(config(package_mode="pad"), cpu)
    with pytest.raises(NotImplementedError, match="package_mode"):
        T.InversionTrainer(config(package_mode="window"), cpu)
    # the BiGRU: pad_masked is pad
    a, b = T.InversionTrainer(bigru_config(package_mode="pad_masked"), cpu), T.InversionTrainer(bigru_config(package_mode="pad"), cpu)
    assert isinstance(a.G, BiGRU) and a.padded and b.padded and not T.InversionTrainer(bigru_config(), cpu).padded
    assert T.PADDED_MODES == ("pad", "pad_masked") and set(T.PADDED_MODES) < set(T.PACKAGE_MODES)

    # ... step for step: both modes hand the batch to forward_padded and the masked loss
    class Seen(Exception):
        pass

    def probe(x, lengths):
        raise Seen(tuple(int(n) for n in lengths))

    batch = {"x": torch.zeros(2, 24, 5), "y": torch.zeros(2, 12, 5), "lengths": torch.tensor([5, 3], dtype=torch.int32)}
    for tr2 in (a, b):
        tr2.G.forward_padded = probe
        tr2.steps = 1
        with pytest.raises(Seen, match=r"\(5, 3\)"):
            tr2.train_step(batch)
