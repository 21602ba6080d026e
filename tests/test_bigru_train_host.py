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


@pytest.mark.parametrize("name", list(O.EDGE_SHAPES))
def test_edge_shape_is_admitted_by_the_restatements_own_float32_run(name):
    """The device's bars are exact-fp32 bars: a shape of tests/test_gpu_bigru_train_edges.py is a yardstick only if the restatement's own
    float32 arithmetic is within HALF of every bar against its float64 run, on the scales the device test uses, and the case is kink-free."""
    r32 = O.edge_restatement(name, torch.float32)
    r64 = O.edge_restatement(name, torch.float64)
    assert min(r32["kink"], r64["kink"]) > O.KINK_MARGIN
    errs = O.edge_errors(r32, r64, O.EDGE_SHAPES[name][5])
    assert {"y", "loss", "dx", "running_mean", "running_var"} <= set(errs) and sum(k.startswith("grad.") for k in errs) == 22
    for k, (e, bar) in errs.items():
        assert e <= 0.5 * bar, (k, e)


def test_edge_shapes_reach_what_they_are_there_for():
    """Pure arithmetic on the table: the sizes at which the training kernels' loops and tiles change form (csrc/hificar_bigru_train*.h*)."""
    S = O.EDGE_SHAPES
    tiles = {n: -(-s[4] // 64) for n, s in S.items()}
    assert (tiles["t64"], tiles["t65"], tiles["t129"], tiles["t63_b1"]) == (1, 2, 3, 1) and S["t65"][4] % 64 == S["t129"][4] % 64 == 1
    assert S["o32"][2] == S["o32_tanh"][2] == 32 and S["o32_tanh"][7] and S["o1_tanh"][7] and S["o1_tanh"][2] == 1 and tiles["o1_tanh"] == 2
    assert (S["h128_ns2"][1], S["h192_ns2"][1]) == (128, 192) and all(S[n][6] == 2 and S[n][3] % 2 == 1 for n in ("h128_ns2", "h192_ns2"))
    cin, H, out, B, T, p, ns, tanh = S["stride"]
    assert B * T > 4096 * 256 // 128          # bigru_bn_bwd_dx_kernel: 4096 blocks x 256 elements of B T x 128
    assert B * T * 2 * H > 4096 * 1024        # bigru_dropout_kernel (1024 elements per block) and bigru_hprev_kernel (256 float4)
    assert tiles["stride"] == 3 and T % 64 == 2 and -(-B * T // 32) == 269 and ns is None and 2 * B <= 256
    assert sorted({S[n][5] for n in S}) == [0.3, 0.5, 0.9]
    assert len(set(O.EDGE_SEEDS.values())) == len(S)


# ------------------------------------------------------------------------------------------------
# the mask generator against what dropout is supposed to be (the bounds are binomial, five standard deviations, not measurements)
# ------------------------------------------------------------------------------------------------
MASK_N = 1 << 20
MASK_PS = (0.1, 0.3, 0.5, 0.9)
MASK_SEEDS = (11, 2 ** 61 + 12345)
MASK_OFFSETS = (0, 1, 2 ** 32)


def kept(seed, offset, site, p, n=MASK_N):
    return bigru_dropout_mask(seed, offset, site, (n,), p) > 0


def five_sigma(q, n):
    return 5.0 * np.sqrt(q * (1.0 - q) / n)


@pytest.mark.parametrize("p", MASK_PS)
def test_mask_keep_rate_and_kept_value(p):
    q = 1.0 - float(np.float32(p))
    value = np.float32(1) / (np.float32(1) - np.float32(p))
    for seed in MASK_SEEDS:
        for offset in MASK_OFFSETS:
            for site in BIGRU_DROPOUT_SITES:
                m = bigru_dropout_mask(seed, offset, site, (MASK_N,), p)
                assert m.dtype == np.float32 and set(np.unique(m)) == {np.float32(0), value}, (seed, offset, site)
                assert abs(float((m > 0).mean()) - q) <= five_sigma(q, MASK_N), (seed, offset, site)


@pytest.mark.parametrize("p", MASK_PS)
def test_masks_of_different_streams_are_independent(p):
    """Two masks that differ only in site, only in offset or only in seed: both keep a position with probability (1 - p)^2."""
    q2 = (1.0 - float(np.float32(p))) ** 2
    base = (MASK_SEEDS[0], 0, 0)
    pairs = [((s, 0, a), (s, 0, b)) for s in MASK_SEEDS for a, b in ((0, 1), (0, 2), (1, 2))]
    pairs += [((s, a, 2), (s, b, 2)) for s in MASK_SEEDS for a, b in ((0, 1), (0, 2 ** 32), (1, 2 ** 32), (1, 2))]
    pairs += [(base, (MASK_SEEDS[1], 0, 0)), (base, (MASK_SEEDS[0] + 1, 0, 0)), (base, (MASK_SEEDS[0] ^ (1 << 63), 0, 0))]
    for u, v in pairs:
        both = float((kept(*u, p) & kept(*v, p)).mean())
        assert abs(both - q2) <= five_sigma(q2, MASK_N), (u, v, both)


@pytest.mark.parametrize("p", MASK_PS)
def test_mask_is_independent_along_the_stream(p):
    """Positions e and e + k are both kept with probability (1 - p)^2, at the lags of the float4 lanes (1, 2), the next float4 (4) and the
    row strides 128 (fc1) and 2H = 512.  (Overlapping pairs share elements, so the share's true deviation is up to 1.4 binomial ones: the
    bound is tighter than five of its own.)"""
    q2 = (1.0 - float(np.float32(p))) ** 2
    for seed in MASK_SEEDS:
        for site in BIGRU_DROPOUT_SITES:
            k0 = kept(seed, 0, site, p)
            for lag in (1, 2, 4, 128, 512):
                both = float((k0[:-lag] & k0[lag:]).mean())
                assert abs(both - q2) <= five_sigma(q2, MASK_N - lag), (seed, site, lag, both)


def test_mask_at_degenerate_probabilities():
    """p = 0 (and anything not above it) is the identity and draws nothing.  u is a multiple of 2^-24, and an element is kept when u >= p in
    float32: for 0 < p <= 2^-24 exactly the elements whose 24 bits are all zero (u = 0) are dropped — the keep set of p = 2^-24 — and below
    2^-25 the kept value 1 / (1 - p) is exactly 1 in float32."""
    for p in (0.0, -0.0, -0.5):
        assert np.array_equal(bigru_dropout_mask(3, 7, "gru2", (5, 4, 3), p), np.ones((5, 4, 3), np.float32))
    tiny = bigru_dropout_mask(11, 0, "fc1", (MASK_N,), 1e-8)
    edge = bigru_dropout_mask(11, 0, "fc1", (MASK_N,), 2.0 ** -24)
    assert set(np.unique(tiny)) <= {np.float32(0), np.float32(1)}
    assert np.array_equal(tiny > 0, edge > 0)
    assert set(np.unique(edge)) <= {np.float32(0), np.float32(1) / (np.float32(1) - np.float32(2.0 ** -24))}
    dropped = int((tiny == 0).sum())  # expected MASK_N / 2^24 = 1 / 16 of an element; five deviations (0.25 each) above that is below 2
    assert dropped <= 1
    # ... and a stretch that does hold such an element: the first u = 0 of this stream, found through p = 2^-23 (drops u in {0, 2^-24})
    wide = bigru_dropout_mask(11, 0, "fc1", (1 << 24,), 2.0 ** -23) == 0
    low = bigru_dropout_mask(11, 0, "fc1", (1 << 24,), 1e-8) == 0
    assert not (low & ~wide).any() and 0 < int(wide.sum()) < 40 and int(low.sum()) <= int(wide.sum())


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
