"""Host-side checks of BiGRU training on ragged batches (``pytest -m "not gpu"``): the CPU restatement tests/bigru_ragged_oracle.py (admission
of every shape of tests/test_gpu_bigru_ragged.py, and that it is what it claims to be), ``masked_l1_loss``, the length-bucketed batch
sampler, the ``pad`` collater and the trainer's acceptance of ``package_mode: pad``.
"""

import os
import subprocess

import numpy as np
import pytest
import torch

import bigru_ragged_oracle as R
import bigru_train_oracle as O
from conftest import REPO
from articulatory_amd import _native
from articulatory_amd.bin import train as T
from articulatory_amd.losses import masked_l1_loss
from articulatory_amd.utils.synth import uniform


@pytest.mark.parametrize("name", list(R.RAGGED_SHAPES))
def test_ragged_shape_is_admitted_by_the_restatements_own_float32_run(name):
    """The admission rule of tests/test_bigru_train_host.py on the ragged shapes: the restatement's own float32 run within HALF of every bar
    of its float64 run, kink-free on the valid frames; and the definition's zeros: y and dx on padded frames."""
    r32 = R.ragged_restatement(name, torch.float32)
    r64 = R.ragged_restatement(name, torch.float64)
    assert min(r32["kink"], r64["kink"]) > O.KINK_MARGIN
    p, lengths, T_ = R.RAGGED_SHAPES[name][7], R.RAGGED_SHAPES[name][6], R.RAGGED_SHAPES[name][5]
    errs = O.edge_errors(r32, r64, p)
    assert {"y", "loss", "dx", "running_mean", "running_var"} <= set(errs) and sum(k.startswith("grad.") for k in errs) == 22
    print(name, "worst share of a bar:", max(e / bar for e, bar in errs.values()), "kink", r64["kink"])
    for k, (e, bar) in errs.items():
        assert e <= 0.5 * bar, (k, e)
    pad = ~R.valid_mask(lengths, T_)
    for r in (r32, r64):
        assert float(r["y"].transpose(1, 2)[pad].abs().max() if pad.any() else 0.0) == 0.0
        assert float(r["dx"].transpose(1, 2)[pad].abs().max() if pad.any() else 0.0) == 0.0


def test_shapes_reach_what_they_are_there_for():
    S = R.RAGGED_SHAPES
    assert sorted(S["mixed"][6]) == [0, 1, 5, 9] and S["mixed"][5] == 9                      # full, one frame, empty, partial
    assert S["tiles"][6] == (130, 64, 65) and S["tiles"][3]                                  # on a head-tile edge, one past it, tanh'
    assert all(S[n][8] == 2 and S[n][4] % 2 == 1 for n in ("ns2", "h192", "h256_ns2"))       # pairs of unequal lengths and an odd tail
    assert all(S[n][6][0] != S[n][6][1] for n in ("ns2", "h192", "h256_ns2"))
    cin, H, out, tanh, B, T_, lengths, p, ns = S["stride"]
    # bigru_bn_bwd_dx_kernel: 4096 blocks x 256 elements of B T x 128; bigru_zero_pad_kernel: 8 blocks x 256 float4 per sequence; 269 rows
    # per batch-norm lane, valid and padded ones mixed in every lane
    assert B * T_ > 4096 * 256 // 128 and (T_ - min(lengths)) * (2 * H // 4) > 8 * 256 and -(-B * T_ // 32) == 269
    assert min(lengths) == 0 and max(lengths) == T_ and len(set(lengths)) == B
    assert len(set(R.RAGGED_SEEDS.values())) == len(S) and set(R.RAGGED_SEEDS) == set(S)
    assert all(sum(s[6]) >= 2 and len(s[6]) == s[4] for s in S.values())


def test_each_sequence_of_a_ragged_batch_is_that_sequence_alone():
    params, sd, x, _, lengths, _ = R.ragged_case("mixed")
    o = R.BiGRURaggedOracle(sd, dropout=params["dropout"], dtype=torch.float64)
    with torch.no_grad():
        y = o.gru_outputs(x, lengths)
        for b, n in enumerate(lengths):
            if n == 0:
                assert float(y[b].abs().max()) == 0.0
                continue
            alone, _ = o.grus[0](torch.from_numpy(x[b:b + 1, :, :n]).double().transpose(1, 2))
            assert float((y[b, :n] - alone[0]).abs().max()) < 1e-14
            assert float(y[b, n:].abs().max() if n < y.shape[1] else 0.0) == 0.0


def test_one_full_sequence_is_the_dense_restatement():
    params, sd, x, t, _, _ = R.ragged_case("b1")
    a = R.BiGRURaggedOracle(sd, dropout=params["dropout"], dtype=torch.float64)
    b = O.BiGRUTrainOracle(sd, dropout=params["dropout"], dtype=torch.float64)
    ya, la, ga, dxa = a.loss_and_grads_padded(x, t, (x.shape[2],))
    yb, lb, gb, dxb = b.loss_and_grads(x, t)
    assert float((ya - yb).abs().max()) < 1e-13 and abs(float(la) - float(lb)) < 1e-13 and float((dxa - dxb).abs().max()) < 1e-13
    for k in gb:
        assert float((ga[k] - gb[k]).abs().max()) < 1e-12, k
    assert float((a.running_var - b.running_var).abs().max()) < 1e-14 and a.num_batches_tracked == b.num_batches_tracked


def test_masked_l1_loss_against_a_loop():
    B, C, T_ = 4, 3, 9
    lengths = (9, 1, 0, 5)
    a = torch.from_numpy(uniform(1, "a", (B, C, T_), -1.0, 1.0)).double().requires_grad_(True)
    b = torch.from_numpy(uniform(1, "b", (B, C, T_), -1.0, 1.0)).double()
    b[1, :, 1:] = float("nan")  # what the padding holds does not matter
    total = 0.0
    for i, n in enumerate(lengths):
        for c in range(C):
            for t in range(n):
                total += abs(float(a.detach()[i, c, t]) - float(b[i, c, t]))
    loss = masked_l1_loss(a, b, torch.tensor(lengths, dtype=torch.int32))
    assert abs(float(loss.detach()) - total / (sum(lengths) * C)) < 1e-14
    assert abs(float(loss) - float(R.masked_l1(a.detach(), torch.nan_to_num(b), lengths))) < 1e-14
    loss.backward()
    pad = ~R.valid_mask(lengths, T_)
    assert torch.isfinite(a.grad).all() and float(a.grad.transpose(1, 2)[pad].abs().max()) == 0.0
    assert torch.equal(a.grad.transpose(1, 2)[~pad].abs(), torch.full((sum(lengths), C), 1.0 / (sum(lengths) * C), dtype=torch.float64))
    full = masked_l1_loss(a.detach().float(), torch.nan_to_num(b).float(), [T_] * B)
    assert abs(float(full) - float(torch.nn.functional.l1_loss(a.detach().float(), torch.nan_to_num(b).float()))) < 1e-6
    with pytest.raises(RuntimeError, match="entries"):
        masked_l1_loss(a, b, [1, 2])


FIXED_LENGTHS = [int(n) for n in np.random.default_rng(5).integers(20, 600, size=203)]


def test_bucket_sampler_covers_repeats_and_pads_less():
    s = T.LengthBucketBatchSampler(FIXED_LENGTHS, batch_size=8, bucket_batches=4, seed=3, drop_last=False)
    batches = list(s)
    assert sorted(i for b in batches for i in b) == list(range(203)) and len(batches) == len(s)  # every utterance exactly once
    d = T.LengthBucketBatchSampler(FIXED_LENGTHS, batch_size=8, bucket_batches=4, seed=3, drop_last=True)
    full = list(d)
    assert len(full) == len(d) and all(len(b) == 8 for b in full) and len(set(i for b in full for i in b)) == 8 * len(full)
    again = T.LengthBucketBatchSampler(FIXED_LENGTHS, batch_size=8, bucket_batches=4, seed=3, drop_last=False)
    assert list(again) == batches                               # seeded: epoch 0 twice
    assert list(again) != batches and again.batches(0) == batches  # the next epoch is another order; an epoch is a pure function of its number
    assert T.LengthBucketBatchSampler(FIXED_LENGTHS, 8, 4, seed=4, drop_last=False).batches(0) != batches
    # sorting pools cannot pad more than not sorting them: bucket_batches = 1 is the plain shuffled order of the same permutation
    plain = T.LengthBucketBatchSampler(FIXED_LENGTHS, batch_size=8, bucket_batches=1, seed=3, drop_last=False).batches(0)
    unsorted = [sorted(b) for b in plain]
    assert T.padded_share(FIXED_LENGTHS, batches) <= T.padded_share(FIXED_LENGTHS, unsorted)
    assert T.padded_share(FIXED_LENGTHS, T.LengthBucketBatchSampler(FIXED_LENGTHS, 8, 16, seed=3).batches(0)) < 0.5 * T.padded_share(FIXED_LENGTHS, unsorted)
    assert T.padded_share([5, 5, 3], [[0, 1], [2]]) == 0.0 and abs(T.padded_share([4, 2], [[0, 1]]) - 0.25) < 1e-15


def test_pad_collater_pads_with_zeros_and_cuts_long_utterances():
    rng = np.random.default_rng(0)
    items = [(rng.standard_normal((n, 5)).astype(np.float32) + 3.0, rng.standard_normal((n, 3)).astype(np.float32) + 3.0) for n in (40, 7, 24)]
    b = T.PadCollater()(items)
    assert b["x"].shape == (3, 5, 40) and b["y"].shape == (3, 3, 40) and b["x"].dtype == torch.float32
    assert b["lengths"].dtype == torch.int32 and b["lengths"].tolist() == [40, 7, 24]
    for i, (a, c) in enumerate(items):
        n = len(a)
        assert np.array_equal(b["x"][i, :, :n].numpy(), a.T) and np.array_equal(b["y"][i, :, :n].numpy(), c.T)
        assert float(b["x"][i, :, n:].abs().sum()) == 0.0 and float(b["y"][i, :, n:].abs().sum()) == 0.0
    c = T.PadCollater(pad_max_frames=20, seed=1)(items)
    assert c["x"].shape == (3, 5, 20) and c["lengths"].tolist() == [20, 7, 20]
    for i in (0, 2):  # a window of the utterance, the same one on both sides
        a, t = items[i]
        starts = [s for s in range(len(a) - 20 + 1) if np.array_equal(a[s:s + 20].T, c["x"][i].numpy())]
        assert len(starts) == 1 and np.array_equal(t[starts[0]:starts[0] + 20].T, c["y"][i].numpy())
    ds = T.WindowPairs(synthetic=50, frames=0, dims=(5, 3), seed=0, frames_range=(10, 40))
    counts = [len(a) for a, _ in ds.items]
    assert min(counts) >= 10 and max(counts) <= 40 and len(set(counts)) > 5 and all(len(a) == len(t) for a, t in ds.items)
    assert counts == [len(a) for a, _ in T.WindowPairs(synthetic=50, frames=0, dims=(5, 3), seed=0, frames_range=(10, 40)).items]


def base_config(**kw):
    cfg = dict(generator_type="BiGRU", dataset_mode="art", generator_params=dict(in_channels=24, hidden_size=64, out_channels=12),
               generator_optimizer_params=dict(lr=1e-3), generator_scheduler_params=dict(step_size=10, gamma=0.5), train_max_steps=100,
               discriminator_train_start_steps=100)
    cfg.update(kw)
    return cfg


def test_inversion_trainer_accepts_pad_and_still_refuses_the_rest():
    cpu = torch.device("cpu")
    tr = T.InversionTrainer(base_config(package_mode="pad"), cpu)
    assert tr.package_mode == "pad" and tr.steps == 0
    assert T.InversionTrainer(base_config(), cpu).package_mode == "random_window"  # the default is unchanged
    with pytest.raises(NotImplementedError, match="package_mode"):
        T.InversionTrainer(base_config(package_mode="window"), cpu)
    with pytest.raises(ValueError, match="lengths"):
        tr.train_step({"x": torch.zeros(2, 24, 5), "y": torch.zeros(2, 12, 5)})
    with pytest.raises(NotImplementedError, match="discriminator_train_start_steps = 50 is below train_max_steps = 100"):
        T.InversionTrainer(base_config(package_mode="pad", discriminator_train_start_steps=50), cpu)
    with pytest.raises(NotImplementedError, match="dataset_mode in art / a2m / m2a"):
        T.InversionTrainer(base_config(package_mode="pad", dataset_mode="a2w"), cpu)
    with pytest.raises(NotImplementedError, match="use_stft_loss"):
        T.InversionTrainer(base_config(package_mode="pad", use_stft_loss=True), cpu)
    with pytest.raises(NotImplementedError, match="use_ar"):
        T.InversionTrainer(base_config(package_mode="pad", generator_params=dict(in_channels=24, hidden_size=64, out_channels=12, use_ar=True)), cpu)


def test_forward_padded_refuses_before_it_needs_a_device():
    """The refusals that need no GPU: a CPU tensor in train() mode (no fallback), and eval mode routes to forward(lengths=)."""
    from articulatory_amd.models import BiGRU

    m = BiGRU(in_channels=8, hidden_size=64, out_channels=12).train()
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        m.forward_padded(torch.zeros(2, 8, 5), [5, 3])
    with pytest.raises(NotImplementedError, match="forward_padded"):  # forward(lengths=) in train() mode points to it
        m(torch.zeros(2, 8, 5), lengths=[5, 3])
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m.eval().forward_padded(torch.zeros(2, 8, 5), [5, 3])


def test_three_step_batches_are_admitted():
    """The three `pad` steps of tests/test_gpu_bigru_ragged.py's trainer test: the restatement's own float32 losses within half of the
    device's loss bar of its float64 ones (the rule by which tools/make_golden_bigru_train.py picks the five-step run's first batch)."""
    l32, _ = R.run_steps3(torch.float32)
    l64, _ = R.run_steps3(torch.float64)
    errs = [abs(a - b) / abs(b) for a, b in zip(l32, l64)]
    print("three-step float32 against float64:", errs)
    assert max(errs) <= 0.5 * R.STEPS3_LOSS_BAR
    assert all(max(n) == 37 and len(n) == 3 for n in R.STEPS3_LENGTHS)  # every batch padded to the case's T


def test_ragged_entry_point_in_the_header_and_the_binding(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hificar.h"\n'
                   "int use(hificar_bigru* h, const float* x, float* y, void* p, const int32_t* n) {\n"
                   "    return hificar_bigru_forward_train_ragged(h, x, n, n, y, y, 2, 5, 0.3f, 1u, 0u, p, hificar_bigru_tape_bytes(h, 2, 5), p,\n"
                   "                                              hificar_bigru_train_workspace_bytes(h, 2, 5), 0);\n}\n")
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hificar_bigru_forward_train_ragged" in _native.SYMBOLS
    assert hasattr(_native.load_library(), "hificar_bigru_forward_train_ragged")
