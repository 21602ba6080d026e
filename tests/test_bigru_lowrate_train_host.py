"""Host-side checks of BiGRU training on low-rate inputs (``pytest -m "not gpu"``): the adjoint interpolation as the device forms it against
the transpose of the float64 front end, the commutation of layer 1's gradients with the interpolation, the admission of every shape of
tests/test_gpu_bigru_lowrate_train.py, the C entry points' refusals on a handle without a device, the Python method's, and the trainer's
low-rate collaters and config keys.
"""

import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import bigru_lowrate_train_oracle as L
import bigru_train_oracle as O
import predict_ema_oracle as P
from conftest import REPO
from articulatory_amd import _native
from articulatory_amd.bin import train as T
from articulatory_amd.models import BiGRU, Transformer


# ---------------------------------------------------------------------------------------------- the adjoint interpolation
@pytest.mark.parametrize("f", [1, 2, 3, 4, 5, 16])
@pytest.mark.parametrize("l", [1, 2, 3, 7, 33])
def test_adjoint_gather_is_the_transposed_interpolation(f, l):
    rng = np.random.default_rng(100 * f + l)
    d = rng.standard_normal((f * l, 5))
    At = P.interp(np.eye(l), f)  # (l, f l): the transpose of the interpolation matrix, from the float64 front end itself
    assert np.array_equal(At.T, L.interp_matrix(f, l)) and np.abs(At.sum(axis=0) - 1).max() <= 1e-15
    got, used0, used1 = L.adjoint_gather(d, f, l)
    assert np.abs(got - At @ d).max() <= 1e-13 * max(1.0, np.abs(d).max() * 2 * f)
    i0, i1, _ = P.source_index(np.arange(f * l), f, l)
    assert (used0 == 1).all()                      # every frame once with its (1 - lam) weight ...
    assert np.array_equal(used1, (i1 != i0) * 1)   # ... and once with lam where it has a second source frame
    # the runs are contiguous and in order: they tile 0 .. f l - 1 as the frames' i0 (first_frame is where i0 steps)
    assert [L.first_frame(j, f) for j in range(l)] == [int(np.argmax(i0 == j)) if j < l else 0 for j in range(l)]


def test_layer_one_gradients_commute_with_the_interpolation():
    rng = np.random.default_rng(7)
    for f, l, C, G in ((4, 33, 24, 48), (3, 11, 13, 30), (16, 3, 8, 12), (2, 1, 8, 12), (1, 9, 8, 12)):
        X = rng.uniform(-1, 1, (l, C))
        dG = rng.uniform(-1, 1, (f * l, G))
        A = L.interp_matrix(f, l)
        dgl, _, _ = L.adjoint_gather(dG, f, l)
        dW_hi, db_hi = dG.T @ (A @ X), dG.sum(axis=0)
        dW_lo, db_lo = dgl.T @ X, dgl.sum(axis=0)
        assert np.abs(dW_lo - dW_hi).max() <= 1e-12 * np.abs(dW_hi).max(), (f, l)
        assert np.abs(db_lo - db_hi).max() <= 1e-12 * np.abs(dG).sum(axis=0).max(), (f, l)


def test_stretch_is_the_front_end_and_its_gradient_the_adjoint():
    rng = np.random.default_rng(8)
    x = rng.standard_normal((3, 5, 7))
    x[1, :, 4:] = np.nan
    lengths = (7, 4, 0)
    for zs in (False, True):
        xt = torch.from_numpy(x).requires_grad_(not zs)
        y = L.stretch(xt, 3, lengths, zs, torch.float64)
        assert np.abs(y.detach().numpy() - P.front_end(x, lengths, 3, zs)).max() <= 1e-13
    w = torch.from_numpy(rng.standard_normal(tuple(y.shape)))
    xt = torch.from_numpy(x).requires_grad_(True)
    (L.stretch(xt, 3, lengths, False, torch.float64) * w).sum().backward()
    for b, l in enumerate(lengths):
        want, _, _ = L.adjoint_gather(w[b, :, :3 * l].numpy().T, 3, l)
        assert l == 0 or np.abs(xt.grad[b, :, :l].numpy() - want.T).max() <= 1e-13
        assert float(xt.grad[b, :, l:].abs().max() if l < 7 else 0.0) == 0.0  # exactly zero on padded low-rate frames


# ---------------------------------------------------------------------------------------------- admission of the GPU shapes
@pytest.mark.parametrize("name", list(L.LOW_SHAPES))
def test_low_rate_shape_is_admitted_by_the_restatements_own_float32_run(name):
    """The admission rule of tests/test_bigru_train_host.py: the restatement's own float32 run within HALF of every bar of its float64 run,
    kink-free on the valid frames."""
    r32, r64 = L.low_restatement(name, torch.float32), L.low_restatement(name, torch.float64)
    assert min(r32["kink"], r64["kink"]) > O.KINK_MARGIN
    errs = O.edge_errors(r32, r64, L.LOW_SHAPES[name][8])
    zs = L.LOW_SHAPES[name][10]
    assert ("dx" in errs) == (not zs) and sum(k.startswith("grad.") for k in errs) == 22
    print(name, "worst share of a bar:", max(e / bar for e, bar in errs.values()), "kink", r64["kink"])
    for k, (e, bar) in errs.items():
        assert e <= 0.5 * bar, (k, e)
    lengths, f, Tl = L.LOW_SHAPES[name][7], L.LOW_SHAPES[name][5], L.LOW_SHAPES[name][6]
    if lengths is not None:
        pad = torch.arange(Tl)[None, :] >= torch.tensor(lengths)[:, None]
        for r in (r32, r64):
            assert float(r["dx"].transpose(1, 2)[pad].abs().max()) == 0.0
            assert float(r["y"].transpose(1, 2)[pad.repeat_interleave(f, dim=1)].abs().max()) == 0.0


def test_golden_cases_of_the_reference_are_the_float64_restatement():
    """tests/golden/gold_bigru_lowrate_train.npz (the reference's own BiGRU in train() mode on torch's F.interpolate, float64, stored as float32)
    against the restatement: two independent routes to the same step, the low-rate input gradient included."""
    gold = np.load(os.path.join(REPO, "tests", "golden", "gold_bigru_lowrate_train.npz"))
    for name in L.GOLD:
        assert L.LOW_SHAPES[name][7] is None and not L.LOW_SHAPES[name][10]
        assert float(gold[name + "_f32_share_of_bar"]) <= 0.5  # the tool's admission rule
        r = L.low_restatement(name, torch.float64)
        assert abs(float(r["loss"]) - float(gold[name + "_loss"])) <= 1e-9 * abs(float(r["loss"]))
        keys = [k for k in r if k not in ("loss", "kink")]
        assert len(keys) == 26  # y, dx, the running statistics, 22 gradients
        for k in keys:
            assert O.deviation(gold, f"{name}_{k}", r[k]) <= 1e-6, (name, k)  # (float32 storage: 6e-8)


def test_shapes_reach_what_they_are_there_for():
    S = L.LOW_SHAPES
    assert [S[k][5] * S[k][6] for k in ("a16", "a17", "a33")] == [64, 68, 132]       # the head's tile full, with a tail, three deep
    assert S["b_f3"][5] * S["b_f3"][6] == 129 and S["b_f16"][5] == _native.LOWRATE_MAX_FACTOR
    assert (S["c"][0], S["c"][1], S["c"][2], S["c"][5]) == (1024, 256, 18, 4)        # the published model
    assert sorted(S["d"][7]) == [0, 1, 9, 17, 24] and S["d"][6] == 24 and S["e"][9] == 2 and S["d"][7][0] != S["d"][7][1]
    assert S["z"][10] and S["z"][:10] == S["b_f3"][:10]


# ---------------------------------------------------------------------------------------------- the C entry points, without a device
def test_c_entry_points_refuse_bad_arguments_before_the_state():
    lib = _native.load_library()
    hdr = open(os.path.join(REPO, "include", "hificar.h")).read()
    for s in ("hificar_bigru_tape_bytes_lowrate", "hificar_bigru_train_workspace_bytes_lowrate", "hificar_bigru_forward_train_lowrate",
              "hificar_bigru_backward_lowrate"):
        assert s in _native.SYMBOLS and s in hdr and getattr(lib, s)
    h = ctypes.c_void_p()
    cfg = _native.make_bigru_config(dict(in_channels=24, hidden_size=64, out_channels=12, use_tanh=False))
    _native.check(lib.hificar_bigru_create(ctypes.byref(cfg), ctypes.byref(h)), "hificar_bigru_create")
    fake = 1 << 20  # a 256-byte aligned non-null address: every refusal below comes before anything is dereferenced or enqueued
    big = 1 << 40
    lens = np.array([3, 9], dtype=np.int32)
    fn = lib.hificar_bigru_forward_train_lowrate
    err = lib.hificar_last_error

    def call(handle=h, x=fake, lengths=None, host=None, out=fake, stats=fake, B=2, Tl=10, factor=4, zscore=0, p=0.3, tape=fake, tb=big, ws=fake, wb=big):
        return fn(handle, x, lengths, host, out, stats, B, Tl, factor, zscore, p, 1, 0, tape, tb, ws, wb, None)

    try:
        assert call(handle=None) == -1 and call(x=None) == -1 and call(out=None) == -1 and call(stats=None) == -1 and b"null" in err()
        for factor in (0, -1, 17):
            assert call(factor=factor) == -1 and b"factor" in err()
            assert lib.hificar_bigru_tape_bytes_lowrate(h, 2, 10, factor) == 0
        assert call(B=0) == -1 and b"out of range" in err() and call(Tl=0) == -1
        assert call(host=lens.ctypes.data) == -1 and b"lengths_host" in err()
        assert call(lengths=fake) == -1 and b"lengths_host" in err()
        lens[1] = 11
        assert call(lengths=fake, host=lens.ctypes.data) == -1 and b"lengths[1]=11" in err()
        lens[:] = (-1, 9)
        assert call(lengths=fake, host=lens.ctypes.data) == -1 and b"lengths[0]=-1" in err()
        lens[:] = (0, 0)
        assert call(lengths=fake, host=lens.ctypes.data) == -1 and b"more than one valid frame" in err()   # M = 0
        assert call(B=1, Tl=1, factor=1) == -1 and b"more than one valid frame" in err()                   # M = 1, the dense form
        assert call(B=1, Tl=1, factor=1, zscore=1) == -1 and b"more than one valid frame" in err()
        lens[:] = (3, 9)
        assert call(p=1.0) == -1 and b"dropout_p" in err()
        for factor, zscore in ((4, 0), (1, 1), (1, 0)):
            kw = dict(factor=factor, zscore=zscore)
            assert call(tape=fake + 8, **kw) == -1 and b"aligned" in err()
            assert call(ws=fake + 8, **kw) == -1 and b"aligned" in err()
            assert call(ws=None, **kw) == -1
            assert call(tb=lib.hificar_bigru_tape_bytes_lowrate(h, 2, 10, factor) - 1, **kw) == -4 and b"tape too small" in err()
            assert call(wb=1024, **kw) == -4 and b"workspace too small" in err()
            # every argument in order, with and without a tape, on a handle that was never finalized: the state comes last
            assert call(lengths=fake, host=lens.ctypes.data, tb=lib.hificar_bigru_tape_bytes_lowrate(h, 2, 10, factor), **kw) == -2
            assert b"finalize" in err()
            assert call(tape=None, tb=0, **kw) == -2
        bw = lib.hificar_bigru_backward_lowrate
        assert bw(h, fake, 2, 10, 4, 1, fake, big, fake, fake, fake, big, None) == -1 and b"z-scored" in err()   # dx of a zscore tape
        assert bw(h, fake, 2, 10, 17, 0, fake, big, fake, None, fake, big, None) == -1 and b"factor" in err()
        assert bw(h, fake, 2, 10, 4, 0, None, big, fake, None, fake, big, None) == -1 and b"aligned" in err()    # a backward needs its tape
        assert bw(h, fake, 2, 10, 4, 0, fake, 1024, fake, None, fake, big, None) == -4
        assert bw(h, fake, 2, 10, 4, 0, fake, big, fake, None, fake, big, None) == -2
    finally:
        lib.hificar_bigru_destroy(h)


def test_lowrate_tape_shrinks_by_the_input_block_only():
    lib = _native.load_library()
    h = ctypes.c_void_p()
    cfg = _native.make_bigru_config(dict(in_channels=1000, hidden_size=256, out_channels=18, use_tanh=False))
    _native.check(lib.hificar_bigru_create(ctypes.byref(cfg), ctypes.byref(h)), "hificar_bigru_create")

    def rows(B, T):  # bigru_train_rows: 64 rows of slack, whole blocks of 256
        return -(-(B * T + 64) // 256) * 256

    try:
        for B, Tl in ((1, 1), (2, 75), (32, 125), (5, 24)):
            assert lib.hificar_bigru_tape_bytes_lowrate(h, B, Tl, 1) == lib.hificar_bigru_tape_bytes(h, B, Tl)
            for f in (2, 4, 16):
                dense, low = lib.hificar_bigru_tape_bytes(h, B, f * Tl), lib.hificar_bigru_tape_bytes_lowrate(h, B, Tl, f)
                assert dense - low == (rows(B, f * Tl) - rows(B, Tl)) * 1024 * 4, (B, Tl, f)   # [rows][Cin rounded up to 32] floats
        # (f - 1) / f of the input block where the row counts are whole blocks: B Tl + 64 = 256 k and B f Tl + 64 = 256 k'
        B, Tl, f = 1, 192, 4
        block = rows(B, f * Tl) * 1024 * 4
        assert rows(B, Tl) == 256 and rows(B, f * Tl) == 1024
        assert lib.hificar_bigru_tape_bytes(h, B, f * Tl) - lib.hificar_bigru_tape_bytes_lowrate(h, B, Tl, f) == block * (f - 1) // f
        # the workspace sizes need the training state, so a device: tests/test_gpu_bigru_lowrate_train.py
        assert lib.hificar_bigru_train_workspace_bytes_lowrate(h, 2, 75, 4) == 0 == lib.hificar_bigru_train_workspace_bytes(h, 2, 300)
    finally:
        lib.hificar_bigru_destroy(h)


# ---------------------------------------------------------------------------------------------- the Python method, without a device
def test_forward_lowrate_train_refusals():
    m = BiGRU(in_channels=13, hidden_size=64, out_channels=12)
    assert list(inspect.signature(m.forward_lowrate_train).parameters) == ["x", "lengths", "interp_factor", "zscore"]
    assert [p.default for p in inspect.signature(m.forward_lowrate_train).parameters.values()][1:] == [None, 1, False]
    assert not hasattr(Transformer, "forward_lowrate_train")
    x = torch.zeros(1, 13, 4)
    for mode in (m.train(), m.eval()):
        for bad in (0, -2, 17, 2.0, "4", None, True):
            with pytest.raises(ValueError, match="interp_factor"):
                mode.forward_lowrate_train(x, interp_factor=bad)
    before = (m._calls, int(m.bn.num_batches_tracked))
    with pytest.raises(NotImplementedError, match="zscore=True.*gradient of the input is not built"):
        m.train().forward_lowrate_train(x.clone().requires_grad_(True), interp_factor=4, zscore=True)
    for kw in (dict(interp_factor=4), dict(interp_factor=1, zscore=True), dict(interp_factor=1), dict(interp_factor=4, lengths=[3])):
        with pytest.raises(NotImplementedError, match="CUDA/HIP tensor"):
            m.train().forward_lowrate_train(x, **kw)
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):  # eval(): forward_lowrate, its own refusal
        m.eval().forward_lowrate_train(x, interp_factor=4)
    assert (m._calls, int(m.bn.num_batches_tracked)) == before  # a refused call draws no mask and tracks no batch
    with pytest.raises(NotImplementedError, match="inference path.*forward_lowrate_train"):
        m.train().forward_lowrate(x, interp_factor=4)


# ---------------------------------------------------------------------------------------------- the trainer
def base_config(**kw):
    c = dict(generator_type="BiGRU", dataset_mode="art", generator_params=dict(in_channels=5, hidden_size=64, out_channels=3),
             generator_optimizer_type="Adam", generator_optimizer_params=dict(lr=1e-3), generator_scheduler_type="StepLR",
             generator_scheduler_params=dict(step_size=10, gamma=0.5), train_max_steps=5, discriminator_train_start_steps=5)
    c.update(kw)
    return c


def pairs(counts, N, seed=0):
    """Utterances whose values name their frame: input a[i] = i (low rate), target b[t] = t."""
    return [(np.repeat(np.arange(n // N, dtype=np.float32)[:, None], 5, axis=1), np.repeat(np.arange(n, dtype=np.float32)[:, None], 3, axis=1))
            for n in counts]


def test_low_rate_windows_are_aligned():
    N = 4
    c = T.LowRateWindowCollater(batch_max_frames=8, aux_context_window=2, factor=N, seed=3)
    b = c(pairs([48, 13, 100, 12], N))
    assert tuple(b["x"].shape) == (4, 5, 3) and tuple(b["y"].shape) == (4, 3, 12) and b["x"].is_contiguous() and b["y"].is_contiguous()
    starts = b["x"][:, 0, 0]
    assert torch.equal(b["y"][:, 0, 0], N * starts)                                   # y starts at N s
    assert torch.equal(b["x"][:, 0, :], starts[:, None] + torch.arange(3.0)) and torch.equal(b["y"][:, 0, :], N * starts[:, None] + torch.arange(12.0))
    assert float(starts[1]) == 0 and float(starts[3]) == 0 and len(set(starts.tolist())) > 1   # 13 // 4 = 3 frames: one place only
    for frames, ctx in ((8, 1), (9, 0), (7, 2)):
        with pytest.raises(ValueError, match="multiple"):
            T.LowRateWindowCollater(frames, ctx, N)
    assert "clamp at the WINDOW" in T.LowRateWindowCollater.__doc__


def test_low_rate_pad_batches():
    N = 4
    items = pairs([48, 7, 100], N) + [(np.zeros((9, 5), np.float32), np.ones((21, 3), np.float32))]  # 9 input frames, 21 // 4 = 5 target blocks
    b = T.LowRatePadCollater(N, pad_max_frames=40, seed=1)(items)
    assert b["lengths"].tolist() == [10, 1, 10, 5] and b["lengths"].dtype == torch.int32              # l = min(len(a), len(b) // N), cut to 40 / 4
    assert tuple(b["x"].shape) == (4, 5, 10) and tuple(b["y"].shape) == (4, 3, 40)
    for i, l in enumerate(b["lengths"].tolist()):
        assert not b["x"][i, :, l:].any() and not b["y"][i, :, N * l:].any()
        if i != 3:
            assert float(b["y"][i, 0, 0]) == N * float(b["x"][i, 0, 0]) and float(b["y"][i, 0, N * l - 1]) == N * float(b["x"][i, 0, l - 1]) + N - 1
    assert float(b["x"][2, 0, 0]) > 0  # the long utterance was cut at a random low-rate start
    assert bool((b["y"][3, :, :20] == 1).all())
    with pytest.raises(ValueError, match="multiple of lowrate_interp_factor"):
        T.LowRatePadCollater(N, pad_max_frames=42)
    whole = T.LowRatePadCollater(N)(items)
    assert whole["lengths"].tolist() == [12, 1, 25, 5] and tuple(whole["y"].shape) == (4, 3, 100)


def test_factor_one_leaves_the_existing_collaters_and_data_alone():
    """Bitwise: the batches of FrameWindowCollater / PadCollater for a fixed seed (written out here as they were before the low-rate keys),
    and the synthetic data of a config without the keys."""
    rng = np.random.default_rng(5)
    items = [(rng.standard_normal((n, 5)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)) for n in (40, 17, 24)]
    b = T.FrameWindowCollater(8, 2, seed=11)(items)
    r = np.random.default_rng(11)
    starts = [int(r.integers(0, len(a) - 12 + 1)) for a, _ in items]
    assert np.array_equal(b["x"].numpy(), np.stack([a[s:s + 12] for (a, _), s in zip(items, starts)]).transpose(0, 2, 1))
    assert np.array_equal(b["y"].numpy(), np.stack([c[s:s + 12] for (_, c), s in zip(items, starts)]).transpose(0, 2, 1))
    p = T.PadCollater(20, seed=11)(items)
    r = np.random.default_rng(11)
    s0, s2 = int(r.integers(0, 40 - 20 + 1)), int(r.integers(0, 24 - 20 + 1))
    assert p["lengths"].tolist() == [20, 17, 20] and np.array_equal(p["x"][0].numpy(), items[0][0][s0:s0 + 20].T)
    assert np.array_equal(p["y"][2].numpy(), items[2][1][s2:s2 + 20].T) and np.array_equal(p["x"][1, :, :17].numpy(), items[1][0].T)
    a, b1 = T.WindowPairs(synthetic=3, frames=16, dims=(5, 3), seed=2), T.WindowPairs(synthetic=3, frames=16, dims=(5, 3), seed=2, x_factor=1)
    r = np.random.default_rng(2)
    for (x, y), (x1, y1) in zip(a.items, b1.items):
        wx, wy = r.standard_normal((16, 5)).astype(np.float32), np.tanh(r.standard_normal((16, 3))).astype(np.float32)
        assert np.array_equal(x, wx) and np.array_equal(y, wy) and np.array_equal(x1, wx) and np.array_equal(y1, wy)
    low = T.WindowPairs(synthetic=3, frames=18, dims=(5, 3), seed=2, x_factor=4)   # --synthetic draws low-rate inputs
    assert [(len(x), len(y)) for x, y in low.items] == [(4, 16)] * 3


def test_trainer_takes_the_keys_for_the_bigru_and_refuses_the_transformer(caplog):
    cpu = torch.device("cpu")
    with caplog.at_level("INFO"):
        tr = T.InversionTrainer(base_config(lowrate_interp_factor=4), cpu)
    assert (tr.low_factor, tr.low_zscore, tr.lowrate) == (4, False, True)
    assert "lowrate_interp_factor 4" in caplog.records[0].getMessage()
    tr = T.InversionTrainer(base_config(), cpu)
    assert (tr.low_factor, tr.low_zscore, tr.lowrate) == (1, False, False)
    assert T.InversionTrainer(base_config(lowrate_zscore=True, package_mode="pad"), cpu).lowrate
    xp = dict(in_channels=5, out_channels=3, elayers=1, hidden_dim=128)
    for kw in (dict(lowrate_interp_factor=4), dict(lowrate_zscore=True)):
        with pytest.raises(NotImplementedError, match="built for generator_type BiGRU \\(got Transformer\\)"):
            T.InversionTrainer(base_config(generator_type="Transformer", generator_params=xp, **kw), cpu)
    T.InversionTrainer(base_config(generator_type="Transformer", generator_params=xp, lowrate_interp_factor=1), cpu)  # the defaults are no request
    for bad in (0, 17, 2.5):
        with pytest.raises(ValueError, match="interp_factor"):
            T.InversionTrainer(base_config(lowrate_interp_factor=bad), cpu)
