"""BiGRU training on ragged batches of whole utterances on a MI355X: ``BiGRU.forward_padded`` + ``masked_l1_loss`` through
``hificar_bigru_forward_train_ragged`` / ``hificar_bigru_backward`` against the float64 restatement tests/bigru_ragged_oracle.py (shapes and
their CPU admission: ``RAGGED_SHAPES``, tests/test_bigru_ragged_host.py), bitwise against the dense path when nothing is padded, bitwise
independence of whatever padded frames and scratch hold, and the trainer's ``package_mode: pad``.  The bars are those of
tests/test_gpu_bigru_train.py.  ``pytest -m gpu``.
"""

import ctypes
import functools

import numpy as np
import pytest
import torch

import bigru_ragged_oracle as R
import bigru_train_oracle as O
from conftest import rel_err
from test_gpu_bigru_train import TOL_GRAD, TOL_LOSS, TOL_OUT, build, dev, steps_config
from test_gpu_bigru_train_edges import owned, owned_floats
from articulatory_amd import _native
from articulatory_amd.bin.train import InversionTrainer
from articulatory_amd.losses import masked_l1_loss
from articulatory_amd.models import BiGRU
from articulatory_amd.models.bigru import FC1_DIM, _grad_layout
from articulatory_amd.utils.synth import uniform

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(name):
    return R.ragged_restatement(name, torch.float64)  # computed once per shape, never modified


def rstep(m, x, t, lengths, need_dx=True):
    """One forward_padded + backward of the masked L1 loss on the device: (y, loss, {key: grad}, dx)."""
    for p in m.parameters():
        p.grad = None
    xt = dev(x).requires_grad_(need_dx)
    y = m.forward_padded(xt, lengths)
    loss = masked_l1_loss(y, dev(t), lengths)
    loss.backward()
    return y.detach(), loss.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}, xt.grad


def padded(t, lengths):
    """The padded frames of a (B, C, T) tensor, as rows."""
    return t.transpose(1, 2)[~R.valid_mask(lengths, t.shape[2]).to(t.device)]


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", list(R.RAGGED_SHAPES))
def test_ragged_shape_against_float64_restatement(name, monkeypatch):
    assert (O.EDGE_BARS["out"], O.EDGE_BARS["loss"], O.EDGE_BARS["grad"]) == (TOL_OUT, TOL_LOSS, TOL_GRAD)
    params, sd, x, t, lengths, ns = R.ragged_case(name)
    if ns is not None:
        monkeypatch.setenv("HIFICAR_BIGRU_NS", str(ns))
    ref = reference(name)
    assert ref["kink"] > O.KINK_MARGIN
    m = build(params, sd)
    y, loss, grads, dx = rstep(m, x, t, lengths)
    assert y.shape == ref["y"].shape and y.dtype == torch.float32 and dx.shape == ref["dx"].shape
    got = dict(y=y, loss=loss, dx=dx, running_mean=m.bn.running_mean, running_var=m.bn.running_var)
    got.update({"grad." + k: g for k, g in grads.items()})
    errs = O.edge_errors(got, ref, params["dropout"])
    assert sorted(k for k in errs if k.startswith("grad.")) == sorted("grad." + k for k in grads)
    worst = max((k for k in errs if k.startswith("grad.")), key=lambda k: errs[k][0])
    print(f"{name}: y {errs['y'][0]:.3g}, loss {errs['loss'][0]:.3g}, running_mean {errs['running_mean'][0]:.3g}, "
          f"running_var {errs['running_var'][0]:.3g}, dx {errs['dx'][0]:.3g}, worst grad {worst} {errs[worst][0]:.3g}")
    for k, (e, bar) in errs.items():
        assert e < bar, (k, e)
    if sum(lengths) < len(lengths) * x.shape[2]:
        assert float(padded(y, lengths).abs().max()) == 0.0 and float(padded(dx, lengths).abs().max()) == 0.0  # exactly zero
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    assert int(m.bn.num_batches_tracked) == int(sd["bn.num_batches_tracked"]) + 1
    assert "libhificar.so" in open("/proc/self/maps").read()


# ------------------------------------------------------------------------------------------------ the C entry points on owned buffers
def native_step(m, x, dout, p, fill, lengths=None, with_tape=True):
    """hificar_bigru_forward_train (lengths None) or hificar_bigru_forward_train_ragged, then hificar_bigru_backward with a tape; every scratch
    and output buffer pre-filled with ``fill`` bytes: (out, batch statistics, grads, dx)."""
    lib, h = m._lib, m._handle
    B, C, T = x.shape
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = owned_floats((B, m._params["out_channels"], T), fill)
    stats = owned_floats((2, FC1_DIM), fill)
    ws, ws_ptr, ws_bytes = owned(lib.hificar_bigru_train_workspace_bytes(h, B, T), fill)
    tape, tape_ptr, tape_bytes = owned(lib.hificar_bigru_tape_bytes(h, B, T), fill) if with_tape else (None, None, 0)
    tail = (B, T, float(p), 4242, 3, tape_ptr, tape_bytes, ws_ptr, ws_bytes, stream)
    if lengths is None:
        _native.check(lib.hificar_bigru_forward_train(h, x.data_ptr(), out.data_ptr(), stats.data_ptr(), *tail), "hificar_bigru_forward_train")
    else:
        host = torch.tensor(list(lengths), dtype=torch.int32)
        on_dev = host.to("cuda:0")
        _native.check(lib.hificar_bigru_forward_train_ragged(h, x.data_ptr(), on_dev.data_ptr(), host.data_ptr(), out.data_ptr(), stats.data_ptr(), *tail),
                      "hificar_bigru_forward_train_ragged")
    if not with_tape:
        torch.cuda.synchronize()
        return out, stats, None, None
    grads = owned_floats((int(lib.hificar_bigru_grad_floats(h)),), fill)
    dx = owned_floats((B, C, T), fill)
    _native.check(lib.hificar_bigru_backward(h, dout.data_ptr(), B, T, tape_ptr, tape_bytes, grads.data_ptr(), dx.data_ptr(), ws_ptr, ws_bytes, stream),
                  "hificar_bigru_backward")
    torch.cuda.synchronize()
    return out, stats, grads, dx


def native_model(name, B=None, T=None):
    params, sd, x, t, lengths, ns = R.ragged_case(name)
    seed = R.RAGGED_SEEDS[name]
    B, T = B or x.shape[0], T or x.shape[2]
    m = build(params, sd)
    m._native_handle(train=True)
    x = dev(uniform(seed, "x", (B, params["in_channels"], T), -1.0, 1.0))
    dout = dev(uniform(seed, "dout", (B, params["out_channels"], T), -1.0, 1.0))
    return m, params, x, dout, lengths


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("name,B,T", [("mixed", 3, 9), ("h256", 2, 40)])
def test_all_lengths_full_is_bitwise_the_dense_path(name, B, T):
    m, params, x, dout, _ = native_model(name, B, T)
    dense = native_step(m, x, dout, params["dropout"], 0x00)
    ragged = native_step(m, x, dout, params["dropout"], 0x00, lengths=[T] * B)
    assert torch.equal(dense[0], ragged[0]), "out"
    assert torch.equal(dense[1], ragged[1]), "batch statistics"
    assert torch.equal(dense[3], ragged[3]), "dx"
    for key, off, num in _grad_layout(m):
        assert torch.equal(dense[2][off:off + num], ragged[2][off:off + num]), key
        assert float(dense[2][off:off + num].abs().max()) > 0, key
    light = native_step(m, x, dout, params["dropout"], 0x00, lengths=[T] * B, with_tape=False)
    assert torch.equal(light[0], dense[0]) and torch.equal(light[1], dense[1])


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", ["mixed", "tiles", "h256_ns2"])
def test_results_depend_neither_on_padded_frames_nor_on_scratch(name, monkeypatch):
    """x and dout zero in the padded frames on zero-filled buffers, against x and dout NaN there on 0xFF-filled buffers (tape, workspace,
    out, statistics, gradient buffer, dx): finite and bitwise equal, with and without a tape."""
    if R.RAGGED_SHAPES[name][8] is not None:
        monkeypatch.setenv("HIFICAR_BIGRU_NS", str(R.RAGGED_SHAPES[name][8]))
    m, params, x, dout, lengths = native_model(name)
    pad = (~R.valid_mask(lengths, x.shape[2])).to("cuda:0")[:, None, :]
    assert bool(pad.any())
    p = params["dropout"]
    xz, dz = x.masked_fill(pad, 0.0).contiguous(), dout.masked_fill(pad, 0.0).contiguous()
    xn, dn = x.masked_fill(pad, float("nan")).contiguous(), dout.masked_fill(pad, float("nan")).contiguous()
    clean = native_step(m, xz, dz, p, 0x00, lengths=lengths)
    dirty = native_step(m, xn, dn, p, 0xFF, lengths=lengths)
    assert torch.isnan(owned_floats((4,), 0xFF)).all()
    layout = _grad_layout(m)
    for what, a, b in zip(("out", "batch statistics", None, "dx"), clean, dirty):
        if what is None:
            continue
        assert torch.isfinite(b).all(), what
        assert torch.equal(a, b), what
    for key, off, num in layout:
        assert torch.isfinite(dirty[2][off:off + num]).all(), key
        assert torch.equal(clean[2][off:off + num], dirty[2][off:off + num]), key
    assert float(padded(dirty[0], lengths).abs().max()) == 0.0 and float(padded(dirty[3], lengths).abs().max()) == 0.0
    assert float(clean[3].abs().max()) > 0 and all(float(clean[2][off:off + num].abs().max()) > 0 for _, off, num in layout)
    light_clean = native_step(m, xz, dz, p, 0x00, lengths=lengths, with_tape=False)
    light_dirty = native_step(m, xn, dn, p, 0xFF, lengths=lengths, with_tape=False)
    assert torch.isfinite(light_dirty[0]).all() and torch.equal(light_clean[0], light_dirty[0])
    assert torch.isfinite(light_dirty[1]).all() and torch.equal(light_clean[1], light_dirty[1])
    assert torch.equal(light_clean[0], clean[0]) and torch.equal(light_clean[1], clean[1])  # the same arithmetic with and without a tape


# ------------------------------------------------------------------------------------------------ 4
def test_repeatable_and_a_small_step_on_the_grown_workspace():
    params, sd, x, t, lengths, _ = R.ragged_case("mixed")
    runs = [rstep(build(params, sd, seed=4242), x, t, lengths) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][3], runs[1][3])
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
    seed, cin, out_ch = R.RAGGED_SEEDS["mixed"], params["in_channels"], params["out_channels"]

    def batch(tag, B, T):
        return uniform(seed, "regrow.x." + tag, (B, cin, T), -1.0, 1.0), uniform(seed, "regrow.t." + tag, (B, out_ch, T), 4.0, 5.0)

    a = build(params, sd, seed=991)
    rstep(a, *batch("large", 6, 130), (130, 1, 64, 0, 65, 99))
    large_ws = a._train_ws_buf.numel()
    ya, la, ga, dxa = rstep(a, *batch("small", 2, 9), (9, 4))
    assert a._train_ws_buf.numel() == large_ws  # grow-only: the small step ran in the large step's buffer
    b = build(params, sd, seed=991)
    b.set_dropout_seed(991, offset=1)
    yb, lb, gb, dxb = rstep(b, *batch("small", 2, 9), (9, 4))
    assert b._train_ws_buf.numel() < large_ws
    assert torch.equal(ya, yb) and torch.equal(dxa, dxb) and torch.equal(la, lb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    assert int(a.bn.num_batches_tracked) == int(b.bn.num_batches_tracked) + 1


# ------------------------------------------------------------------------------------------------ 5
def test_eval_after_a_ragged_step_is_the_eval_path_on_the_updated_statistics():
    params, sd, x, t, lengths, _ = R.ragged_case("mixed")
    m = build(params, sd)
    rstep(m, x, t, lengths)
    o = R.BiGRURaggedOracle(sd, use_tanh=params["use_tanh"], dropout=params["dropout"], dtype=torch.float64)
    o.loss_and_grads_padded(x, t, lengths)  # the same step: its running statistics are what eval mode goes by
    assert rel_err(m.bn.running_var.cpu().numpy(), o.running_var.numpy()) < TOL_OUT
    with torch.no_grad():
        ref = o.forward_padded(x, lengths, train=False)
    m.eval()
    with torch.no_grad():
        y = m(dev(x), lengths=list(lengths))
        assert torch.equal(m.forward_padded(dev(x), lengths), y)  # eval(): forward_padded is forward(lengths=)
    assert rel_err(y.cpu().numpy(), ref.numpy()) < TOL_OUT
    assert float(padded(y, lengths).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 6
def test_refusals():
    params, sd, _, _, _, _ = R.ragged_case("mixed")
    m = build(params, sd)
    x = torch.zeros(2, 8, 5, device="cuda:0")
    before = (m._calls, int(m.bn.num_batches_tracked))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m.forward_padded(x, [1, 0])
    with pytest.raises(RuntimeError, match=r"lengths must lie in \[0, 5\]"):
        m.forward_padded(x, [5, 6])
    with pytest.raises(RuntimeError, match=r"lengths must lie in \[0, 5\]"):
        m.forward_padded(x, [5, -1])
    with pytest.raises(RuntimeError, match="lengths has 3 entries for a batch of 2"):
        m.forward_padded(x, [5, 3, 1])
    with pytest.raises(NotImplementedError, match="forward_padded"):
        m(x, lengths=[5, 3])
    assert (m._calls, int(m.bn.num_batches_tracked)) == before  # a refused call draws no mask and tracks no batch
    # the C entry point checks the host lengths itself, before anything is enqueued
    m._native_handle(train=True)
    lib, h = m._lib, m._handle
    out, stats = torch.zeros(2, 12, 5, device="cuda:0"), torch.zeros(2, FC1_DIM, device="cuda:0")
    ws, ws_ptr, ws_bytes = owned(lib.hificar_bigru_train_workspace_bytes(h, 2, 5), 0)
    for bad in ([1, 0], [5, 6], [-1, 5]):
        host = torch.tensor(bad, dtype=torch.int32)
        on_dev = host.to("cuda:0")
        rc = lib.hificar_bigru_forward_train_ragged(h, x.data_ptr(), on_dev.data_ptr(), host.data_ptr(), out.data_ptr(), stats.data_ptr(), 2, 5, 0.3, 1, 0,
                                                    None, 0, ws_ptr, ws_bytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == -1, bad  # HIFICAR_E_INVALID
    rc = lib.hificar_bigru_forward_train_ragged(h, x.data_ptr(), on_dev.data_ptr(), None, out.data_ptr(), stats.data_ptr(), 2, 5, 0.3, 1, 0, None, 0, ws_ptr,
                                                ws_bytes, None)
    assert rc == -1 and b"lengths_host" in lib.hificar_last_error()


# ------------------------------------------------------------------------------------------------ 7
def pad_config():
    return dict(steps_config(O.case_params("c0")[0]), package_mode="pad", generator_optimizer_params=dict(lr=R.STEPS3["lr"]),
                generator_grad_norm=R.STEPS3["grad_norm"], generator_scheduler_params=dict(step_size=R.STEPS3["step_size"], gamma=R.STEPS3["gamma"]),
                lambda_aux=R.STEPS3["lambda_aux"], train_max_steps=R.STEPS3["n"], discriminator_train_start_steps=R.STEPS3["n"])


def pad_batch(step):
    x, t, lengths = R.steps3_batch(step)
    return {"x": torch.from_numpy(x), "y": torch.from_numpy(t), "lengths": torch.tensor(lengths, dtype=torch.int32)}


def test_three_pad_steps_through_the_trainer():
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in O.case_state_dict("c0").items()}
    tr = InversionTrainer(pad_config(), torch.device("cuda:0"))
    tr.G.load_state_dict(sd, strict=True)
    tr.G.set_dropout_seed(O.DROPOUT_SEED)
    assert tr.optimizer["generator"].defaults.get("fused") is True
    losses = [float(tr.train_step(pad_batch(s))["train/generator_loss"]) for s in range(R.STEPS3["n"])]
    # the same three steps written out: forward_padded, masked_l1_loss, clip, Adam, scheduler
    m = build(O.case_params("c0")[0], O.case_state_dict("c0"))
    opt = torch.optim.Adam(m.parameters(), lr=R.STEPS3["lr"], fused=True)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=R.STEPS3["step_size"], gamma=R.STEPS3["gamma"])
    hand = []
    for s in range(R.STEPS3["n"]):
        b = pad_batch(s)
        loss = masked_l1_loss(m.forward_padded(b["x"].to("cuda:0"), b["lengths"]), b["y"].to("cuda:0"), b["lengths"]) * R.STEPS3["lambda_aux"]
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), R.STEPS3["grad_norm"])
        opt.step()
        sched.step()
        hand.append(float(loss.detach()))
    assert hand == losses
    for (k, va), vb in zip(tr.G.state_dict().items(), m.state_dict().values()):
        assert torch.equal(va, vb), k
    ref, _ = R.run_steps3(torch.float64)
    errs = [abs(a - b) / abs(b) for a, b in zip(losses, ref)]
    print("losses", losses, "errs", errs)
    assert max(errs) < R.STEPS3_LOSS_BAR
    assert tr.steps == R.STEPS3["n"] and int(tr.G.bn.num_batches_tracked) == int(sd["bn.num_batches_tracked"]) + R.STEPS3["n"]


def test_train_cli_in_pad_mode_with_a_dev_set(tmp_path):
    import yaml

    from articulatory_amd.bin import train as T

    cfg = dict(generator_type="BiGRU", dataset_mode="art", format="npy", generator_params=dict(in_channels=24, hidden_size=64, out_channels=12, dropout=0.3),
               generator_optimizer_type="Adam", generator_optimizer_params=dict(lr=1e-3), generator_grad_norm=10, generator_scheduler_type="StepLR",
               generator_scheduler_params=dict(step_size=1000, gamma=0.5), use_mel_loss=True, lambda_aux=1.0, batch_size=4, batch_max_steps=8,
               hop_size=1, aux_context_window=1, train_max_steps=3, discriminator_train_start_steps=3, log_interval_steps=1, eval_interval_steps=2,
               package_mode="pad", pad_bucket_batches=2, pad_max_frames=30)
    (tmp_path / "config.yml").write_text(yaml.safe_dump(cfg))
    rng = np.random.default_rng(0)
    lines = {"feats": [], "ema": []}
    for u, n in (("a", 50), ("b", 7), ("c", 1)):
        np.save(tmp_path / f"{u}-feats.npy", rng.standard_normal((n, 24)).astype(np.float32))
        np.save(tmp_path / f"{u}-ema.npy", rng.standard_normal((n, 12)).astype(np.float32))
        lines["feats"].append(f"{u} {tmp_path / (u + '-feats.npy')}")
        lines["ema"].append(f"{u} {tmp_path / (u + '-ema.npy')}")
    (tmp_path / "dev_feats.scp").write_text("\n".join(lines["feats"]) + "\n")
    (tmp_path / "dev_ema.scp").write_text("\n".join(lines["ema"]) + "\n")
    T.main(["--config", str(tmp_path / "config.yml"), "--outdir", str(tmp_path), "--synthetic", "12", "--max-steps", "3", "--verbose", "0",
            "--dev-feats-scp", str(tmp_path / "dev_feats.scp"), "--dev-audio-scp", str(tmp_path / "dev_ema.scp")])
    state = torch.load(tmp_path / "checkpoint-3steps.pkl", map_location="cpu")
    assert state["steps"] == 3 and int(state["model"]["generator"]["bn.num_batches_tracked"]) == 2  # (the reference trains from step 1 on)
    BiGRU(**cfg["generator_params"]).load_state_dict(state["model"]["generator"], strict=True)
    best = torch.load(tmp_path / "best_mel_ckpt.pkl", map_location="cpu")
    assert best["steps"] == 2 and (tmp_path / "best_mel_step.txt").read_text().strip() == "2"
    BiGRU(**cfg["generator_params"]).load_state_dict(best["model"]["generator"], strict=True)
