"""Host-side checks of BiGRU training (``pytest -m "not gpu"``): the CPU restatement tests/bigru_train_oracle.py against the golden vectors of
the REAL reference class in train() mode (tools/make_golden_bigru_train.py), the numpy restatement of the dropout generator, the trainer's
refusals, and the new block of the C header.
"""

import os
import subprocess

import numpy as np
import pytest
import torch

import bigru_train_oracle as O
from conftest import GOLDEN, REPO, rel_err
from articulatory_amd import _native
from articulatory_amd.bin import train as T
from articulatory_amd.utils.synth import BIGRU_DROPOUT_SITES, bigru_dropout_mask, bigru_param_spec

TOL = 2e-5


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "gold_bigru_train.npz"))


@pytest.mark.parametrize("tag", list(O.GOLD_CASES))
def test_restatement_reproduces_the_golden_case(gold, tag):
    params, B, T_, _ = O.case_params(tag)
    assert float(gold[f"{tag}_f32_dev"]) <= TOL and float(gold[f"{tag}_kink"]) >= 1e-4  # the tool's admission, as stored
    o = O.BiGRUTrainOracle(O.case_state_dict(tag), use_tanh=params["use_tanh"], dropout=params["dropout"], dtype=torch.float32)
    x, t = O.case_batch(tag)
    y, loss, grads, dx = o.loss_and_grads(x, t)
    assert rel_err(y.numpy(), gold[f"{tag}_y"]) < TOL
    assert abs(float(loss) - float(gold[f"{tag}_loss"][0])) < TOL * abs(float(gold[f"{tag}_loss"][0]))
    assert O.deviation(gold, f"{tag}_dx", dx) < TOL
    for k, g in grads.items():
        assert O.deviation(gold, f"{tag}_grad.{k}", g) < TOL, k
    assert rel_err(o.running_mean.numpy(), gold[f"{tag}_running_mean"]) < TOL
    assert rel_err(o.running_var.numpy(), gold[f"{tag}_running_var"]) < TOL
    assert o.num_batches_tracked == int(gold[f"{tag}_num_batches_tracked"])


def test_restatement_reproduces_the_five_step_run(gold):
    params = O.case_params("c0")[0]
    o = O.BiGRUTrainOracle(O.case_state_dict("c0"), use_tanh=params["use_tanh"], dropout=params["dropout"], dtype=torch.float32)
    first = int(gold["steps_first_batch"])
    opt = torch.optim.Adam(list(o.params.values()), lr=O.STEPS["lr"])
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=O.STEPS["step_size"], gamma=O.STEPS["gamma"])
    losses = []
    for s in range(O.STEPS["n"]):
        x, t = O.case_batch("c0", first + s)
        loss = torch.nn.functional.l1_loss(o.forward(x), torch.from_numpy(t)) * O.STEPS["lambda_aux"]
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(o.params.values()), O.STEPS["grad_norm"])
        opt.step()
        sched.step()
        losses.append(float(loss.detach()))
    assert max(abs(a - b) / abs(b) for a, b in zip(losses, gold["steps_losses"])) < TOL
    for k, v in o.params.items():
        assert O.deviation(gold, "steps_final." + k, v) < TOL, k
    assert O.deviation(gold, "steps_final.bn.running_mean", o.running_mean) < TOL
    assert O.deviation(gold, "steps_final.bn.running_var", o.running_var) < TOL
    assert o.num_batches_tracked == int(gold["steps_num_batches_tracked"]) == int(O.case_state_dict("c0")["bn.num_batches_tracked"]) + O.STEPS["n"]


def test_mask_generator():
    n, p = 100_000, 0.3
    m = bigru_dropout_mask(11, 0, "gru1", (n,), p)
    assert m.dtype == np.float32 and set(np.unique(m)) == {np.float32(0.0), np.float32(1.0) / (np.float32(1.0) - np.float32(p))}
    keep = float((m > 0).mean())
    assert abs(keep - (1 - p)) < 3 * np.sqrt(p * (1 - p) / n)  # 3 sigma of a binomial keep-rate
    assert np.array_equal(m, bigru_dropout_mask(11, 0, "gru1", (n,), p))  # a pure function of (seed, offset, site, element)
    assert np.array_equal(m.reshape(100, 10, 100), bigru_dropout_mask(11, 0, 0, (100, 10, 100), p))  # ... of the row-major element index
    others = [bigru_dropout_mask(11, 0, "gru2", (n,), p), bigru_dropout_mask(11, 0, "fc1", (n,), p), bigru_dropout_mask(11, 1, "gru1", (n,), p),
              bigru_dropout_mask(12, 0, "gru1", (n,), p)]
    for o in others:  # another site, offset or seed: an independent mask (agreement of two independent masks: 0.7^2 + 0.3^2 = 0.58)
        assert abs(float(((o > 0) == (m > 0)).mean()) - 0.58) < 0.01
    assert np.array_equal(bigru_dropout_mask(11, 5, "fc1", (4, 3), 0.0), np.ones((4, 3), np.float32))  # p = 0: the identity
    assert BIGRU_DROPOUT_SITES == {"gru1": 0, "gru2": 1, "fc1": 2}


def test_key_list_is_the_references():
    keys = open(os.path.join(GOLDEN, "gold_bigru_train_keys.txt")).read().split()
    assert keys == open(os.path.join(GOLDEN, "gold_bigru_keys.txt")).read().split()
    spec = bigru_param_spec(in_channels=24, hidden_size=64, out_channels=12, use_tanh=False)
    assert keys == list(spec)


def base_config(**kw):
    cfg = dict(generator_type="BiGRU", dataset_mode="art", generator_params=dict(in_channels=24, hidden_size=64, out_channels=12),
               generator_optimizer_params=dict(lr=1e-3), generator_scheduler_params=dict(step_size=10, gamma=0.5), train_max_steps=100,
               discriminator_train_start_steps=100)
    cfg.update(kw)
    return cfg


def test_inversion_trainer_refusals():
    cpu = torch.device("cpu")
    with pytest.raises(NotImplementedError, match="discriminator_train_start_steps = 50 is below train_max_steps = 100"):
        T.InversionTrainer(base_config(discriminator_train_start_steps=50), cpu)
    with pytest.raises(NotImplementedError, match="discriminator_train_start_steps = 0 is below"):
        cfg = base_config()
        del cfg["discriminator_train_start_steps"]
        T.InversionTrainer(cfg, cpu)
    with pytest.raises(NotImplementedError, match="dataset_mode in art / a2m / m2a"):
        T.InversionTrainer(base_config(dataset_mode="a2w"), cpu)
    with pytest.raises(NotImplementedError, match="generator_type BiGRU"):
        T.InversionTrainer(base_config(generator_type="HiFiGANGenerator"), cpu)
    with pytest.raises(NotImplementedError, match="use_stft_loss"):
        T.InversionTrainer(base_config(use_stft_loss=True), cpu)
    with pytest.raises(NotImplementedError, match="use_ar"):
        T.InversionTrainer(base_config(generator_params=dict(in_channels=24, hidden_size=64, out_channels=12, use_ar=True)), cpu)
    with pytest.raises(NotImplementedError, match="InversionTrainer"):  # the GAN trainer points at the right class
        T.Trainer(base_config(), cpu)
    for mode in T.INVERSION_MODES:  # every supported mode builds (parameters on the CPU: nothing touches a device before the first step)
        tr = T.InversionTrainer(base_config(dataset_mode=mode), cpu)
        assert tr.steps == 0 and set(tr.optimizer) == {"generator"}


def test_window_collater_cuts_equal_windows_from_both_sides():
    rng = np.random.default_rng(0)
    items = [(rng.standard_normal((n, 5)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)) for n in (40, 25, 24)]
    col = T.FrameWindowCollater(batch_max_frames=20, aux_context_window=2, seed=1)  # CollaterMelArt: 20 + 2 * 2 frames
    b = col(items)
    assert b["x"].shape == (3, 5, 24) and b["y"].shape == (3, 3, 24)
    for i, (a, c) in enumerate(items):
        starts = [s for s in range(len(a) - 24 + 1) if np.array_equal(a[s:s + 24].T, b["x"][i].numpy())]
        assert len(starts) == 1 and np.array_equal(c[starts[0]:starts[0] + 24].T, b["y"][i].numpy())  # the same window on both sides
    ds = T.WindowPairs(synthetic=4, frames=30, dims=(5, 3), seed=0)
    assert len(ds) == 4 and ds[0][0].shape == (30, 5) and ds[0][1].shape == (30, 3)


def test_tape_size_without_a_device():
    """As the inference sizes (tests/test_bigru_host.py): a created handle answers without a device.  The tape is pure arithmetic on the
    shape; the training workspace holds weight-gradient partials sized by the chip, so it is only known after hificar_bigru_finalize
    (checked in tests/test_gpu_bigru_train.py)."""
    import ctypes

    lib = _native.load_library()
    h = ctypes.c_void_p()
    cfg = _native.make_bigru_config(dict(in_channels=80, hidden_size=64, out_channels=12, use_tanh=True))
    _native.check(lib.hificar_bigru_create(ctypes.byref(cfg), ctypes.byref(h)), "hificar_bigru_create")
    try:
        rows, H, M = 768, 64, 2 * 300  # B T + 64 rounded up to 256 rows
        # (every piece a multiple of 256 bytes)  header | input rows (96) | two layers' outputs (2H) and gates (8H) | raw fc1 (128) | statistics 3 x 128 | output (B, 12, T)
        assert lib.hificar_bigru_tape_bytes(h, 2, 300) == 256 + rows * (96 + 2 * 2 * H + 2 * 8 * H + 128) * 4 + 3 * 128 * 4 + -(-M * 12 * 4 // 256) * 256
        assert lib.hificar_bigru_tape_bytes(h, 0, 300) == 0
        assert lib.hificar_bigru_train_workspace_bytes(h, 2, 300) == 0  # before finalize: no training state
        assert b"hificar_bigru_finalize" in lib.hificar_last_error()
    finally:
        lib.hificar_bigru_destroy(h)


def test_new_header_block_compiles_as_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hificar.h"\n'
                   "int use(hificar_bigru* h, const float* x, float* y, void* p, const char* const* n, const float* const* d) {\n"
                   "    return hificar_bigru_forward_train(h, x, y, y, 1, 2, 0.3f, 1u, 0u, p, hificar_bigru_tape_bytes(h, 1, 2), p,\n"
                   "                                       hificar_bigru_train_workspace_bytes(h, 1, 2), 0)\n"
                   "         + hificar_bigru_backward(h, x, 1, 2, p, 0, y, 0, p, 0, 0) + hificar_bigru_set_parameters_device(h, n, d, 0, 0)\n"
                   "         + hificar_bigru_grad_count(h) + (int)hificar_bigru_grad_floats(h) + hificar_bigru_grad_info(h, 0, 0, 0, 0);\n}\n")
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name in ("hificar_bigru_set_parameters_device", "hificar_bigru_grad_count", "hificar_bigru_grad_info", "hificar_bigru_grad_floats",
                 "hificar_bigru_tape_bytes", "hificar_bigru_train_workspace_bytes", "hificar_bigru_forward_train", "hificar_bigru_backward"):
        assert name in _native.SYMBOLS
