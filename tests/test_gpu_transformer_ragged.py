"""Transformer training on ragged batches of whole utterances on a MI355X: ``Transformer.forward_padded`` + ``masked_l1_loss`` through
``hificar_xfmr_forward_train_ragged`` / ``hificar_xfmr_backward`` against the float64 restatement tests/transformer_ragged_oracle.py (shapes
and their CPU admission: ``RAGGED_SHAPES``, tests/test_transformer_ragged_host.py), bitwise against the dense path when nothing is padded,
bitwise independence of whatever padded frames and scratch hold, and the trainer's ``package_mode: pad_masked``.  The bars are those of
tests/test_gpu_transformer_train.py (transformer_train_oracle.BARS).  ``pytest -m gpu``.
"""

import ctypes

import numpy as np
import pytest
import torch
import yaml

import transformer_ragged_oracle as R
import transformer_train_oracle as O
from conftest import rel_err
from test_gpu_bigru_train_edges import owned, owned_floats
from test_gpu_transformer_train import assert_within, dev, steps_config
from transformer_oracle import TransformerOracle
from articulatory_amd import _native
from articulatory_amd.bin.train import InversionTrainer
from articulatory_amd.losses import masked_l1_loss
from articulatory_amd.models import Transformer
from articulatory_amd.models.transformer import _grad_layout
from articulatory_amd.utils.synth import uniform

pytestmark = pytest.mark.gpu


def build(params, sd, seed=O.DROPOUT_SEED):
    m = Transformer(**params)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to("cuda:0").train()
    m.set_dropout_seed(seed)
    return m


def padded(t, lengths):
    """The entries of a (B, C, T) tensor on padded frames."""
    return t[(~R.valid_mask(lengths, t.shape[2])).to(t.device)[:, None, :].expand_as(t)]


def rstep(m, x, t, lengths, need_dx=True, gates=None):
    """One forward_padded + masked L1 + backward on the device, in the restatement's result layout.  ``gates``: a dict that receives which
    side of every ReLU the device took (hificar_xfmr_debug_tap), in the restatement's shapes; the taps' padded rows must be zeros."""
    for p in m.parameters():
        p.grad = None
    xt = dev(x).requires_grad_(need_dx)
    bufs = {}
    if gates is not None:
        B, _, T = x.shape
        m._native_handle(train=True)
        for name in O.relu_names(m._params):
            bufs[name] = torch.full((B, T, 3072 if name.endswith("hidden") else m._params["hidden_dim"]), float("nan"), dtype=torch.float32, device="cuda:0")
            m.debug_tap(name, bufs[name])
    y = m.forward_padded(xt, lengths)
    if gates is not None:
        m.debug_tap(None)
        pad = (~R.valid_mask(lengths, x.shape[2])).to("cuda:0")
        for name, buf in bufs.items():
            assert torch.isfinite(buf).all() and float(buf[pad].abs().max() if bool(pad.any()) else 0.0) == 0.0, name
            gates[name] = (buf > 0).cpu() if name.endswith("hidden") else (buf > 0).transpose(1, 2).cpu()
    loss = masked_l1_loss(y, dev(t), lengths)
    loss.backward()
    return dict(out=y.detach(), loss=loss.detach(), dx=xt.grad, grads={k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None},
                stats=m._last_stats.clone(), running={k: v.detach().clone() for k, v in m.named_buffers() if k.endswith(("running_mean", "running_var"))})


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", list(R.RAGGED_SHAPES))
def test_ragged_shape_against_float64_restatement(name):
    params, sd, x, t, lengths = R.ragged_case(name)
    m = build(params, sd)
    before = [int(bn.num_batches_tracked) for bn in m._batch_norms()]
    gates = {}
    got = rstep(m, x, t, lengths, gates=gates)
    ref = R.ragged_restatement(name, torch.float64, gates=gates)
    print(f"  {name}: {ref['gate_flips']} ReLU(s) on the other side than float64's own, the farthest {ref['gate_gap']:.3g} of max |x| from zero")
    assert ref["gate_gap"] < O.GATE_GAP
    assert set(got["grads"]) == set(ref["grads"])
    assert_within(O.errors(got, ref), name)  # (prints the five largest shares of a bar)
    assert torch.isfinite(got["out"]).all() and torch.isfinite(got["dx"]).all()
    if sum(lengths) < x.shape[0] * x.shape[2]:
        assert float(padded(got["out"], lengths).abs().max()) == 0.0 and float(padded(got["dx"], lengths).abs().max()) == 0.0
    assert [int(bn.num_batches_tracked) for bn in m._batch_norms()] == [n + 1 for n in before] and m._calls == 1
    assert "libhificar.so" in open("/proc/self/maps").read()


# ------------------------------------------------------------------------------------------------ the C entry points on owned buffers
def native_step(m, x, dout, p, fill, lengths=None, with_tape=True):
    """hificar_xfmr_forward_train (lengths None) or hificar_xfmr_forward_train_ragged, then hificar_xfmr_backward with a tape; every scratch
    and output buffer pre-filled with ``fill`` bytes: (out, batch statistics, grads, dx)."""
    lib, h = m._lib, m._handle
    B, C, T = x.shape
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = owned_floats((B, m._params["out_channels"], T), fill)
    stats = owned_floats((len(m._batch_norms()), 2, m._params["hidden_dim"]), fill)
    ws, ws_ptr, ws_bytes = owned(lib.hificar_xfmr_train_workspace_bytes(h, B, T), fill)
    tape, tape_ptr, tape_bytes = owned(lib.hificar_xfmr_tape_bytes(h, B, T), fill) if with_tape else (None, None, 0)
    tail = (B, T, float(p), 4242, 3, tape_ptr, tape_bytes, ws_ptr, ws_bytes, stream)
    if lengths is None:
        _native.check(lib.hificar_xfmr_forward_train(h, x.data_ptr(), out.data_ptr(), stats.data_ptr(), *tail), "hificar_xfmr_forward_train")
    else:
        host = torch.tensor(list(lengths), dtype=torch.int32)
        on_dev = host.to("cuda:0")
        _native.check(lib.hificar_xfmr_forward_train_ragged(h, x.data_ptr(), on_dev.data_ptr(), host.data_ptr(), out.data_ptr(), stats.data_ptr(), *tail),
                      "hificar_xfmr_forward_train_ragged")
    if not with_tape:
        torch.cuda.synchronize()
        return out, stats, None, None
    grads = owned_floats((int(lib.hificar_xfmr_grad_floats(h)),), fill)
    dx = owned_floats((B, C, T), fill)
    _native.check(lib.hificar_xfmr_backward(h, dout.data_ptr(), B, T, tape_ptr, tape_bytes, grads.data_ptr(), dx.data_ptr(), ws_ptr, ws_bytes, stream),
                  "hificar_xfmr_backward")
    torch.cuda.synchronize()
    return out, stats, grads, dx


def native_model(name, B=None, T=None):
    params, sd, x, _, lengths = R.ragged_case(name)
    seed = R.RAGGED_SEEDS[name]
    B, T = B or x.shape[0], T or x.shape[2]
    m = build(params, sd)
    m._native_handle(train=True)
    x = dev(uniform(seed, "x", (B, params["in_channels"], T), -1.0, 1.0))
    dout = dev(uniform(seed, "dout", (B, params["out_channels"], T), -1.0, 1.0))
    return m, params, x, dout, lengths


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("name,B,T", [("mixed", 2, 65), ("d96", 2, 130)])  # the dense suite's t65 and d96 sizes (p = 0.2)
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
@pytest.mark.parametrize("name", ["mixed", "tiles", "zero", "d96"])
def test_results_depend_neither_on_padded_frames_nor_on_scratch(name):
    """x and dout zero in the padded frames on zero-filled buffers, against x and dout NaN there on 0xFF-filled buffers (tape, workspace,
    out, statistics, gradient buffer, dx): finite and bitwise equal, with and without a tape."""
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
    # (a conv bias in front of a batch norm has a mathematically zero gradient: rounding may make it exactly 0)
    assert float(clean[3].abs().max()) > 0 and all(float(clean[2][off:off + num].abs().max()) > 0 for k, off, num in layout
                                                   if not k.endswith(O.STEPS_UNCOMPARED))
    light_clean = native_step(m, xz, dz, p, 0x00, lengths=lengths, with_tape=False)
    light_dirty = native_step(m, xn, dn, p, 0xFF, lengths=lengths, with_tape=False)
    assert torch.isfinite(light_dirty[0]).all() and torch.equal(light_clean[0], light_dirty[0])
    assert torch.isfinite(light_dirty[1]).all() and torch.equal(light_clean[1], light_dirty[1])
    assert torch.equal(light_clean[0], clean[0]) and torch.equal(light_clean[1], clean[1])  # the same arithmetic with and without a tape


# ------------------------------------------------------------------------------------------------ 4
def same(a, b):
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["loss"], b["loss"]) and torch.equal(a["dx"], b["dx"]) and torch.equal(a["stats"], b["stats"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


def test_repeatable_and_a_small_step_on_the_grown_workspace():
    params, sd, x, t, lengths = R.ragged_case("mixed")
    same(rstep(build(params, sd, seed=4242), x, t, lengths), rstep(build(params, sd, seed=4242), x, t, lengths))
    seed, cin, out_ch = R.RAGGED_SEEDS["mixed"], params["in_channels"], params["out_channels"]

    def batch(tag, B, T):
        return uniform(seed, "regrow.x." + tag, (B, cin, T), -1.0, 1.0), uniform(seed, "regrow.t." + tag, (B, out_ch, T), 4.0, 5.0)

    a = build(params, sd, seed=991)
    rstep(a, *batch("large", 4, 130), (130, 1, 64, 0))
    large_ws = a._train_ws_buf.numel()
    ra = rstep(a, *batch("small", 2, 9), (9, 4))
    assert a._train_ws_buf.numel() == large_ws  # grow-only: the small step ran in the large step's buffer
    b = build(params, sd, seed=991)
    b.set_dropout_seed(991, offset=1)
    rb = rstep(b, *batch("small", 2, 9), (9, 4))
    assert b._train_ws_buf.numel() < large_ws
    same(ra, rb)
    assert int(a.conv_blocks[0].bn1.num_batches_tracked) == int(b.conv_blocks[0].bn1.num_batches_tracked) + 1


# ------------------------------------------------------------------------------------------------ 5
def test_eval_after_a_ragged_step_is_the_eval_path_on_the_updated_statistics():
    params, sd, x, t, lengths = R.ragged_case("mixed")
    m = build(params, sd)
    rstep(m, x, t, lengths)
    o = R.TransformerRaggedOracle(sd, dtype=torch.float64, dropout=params["dropout"], seed=O.DROPOUT_SEED)
    o.step_padded(x, t, lengths)  # the same step: its running statistics (updated with M / (M - 1)) are what eval mode goes by
    M = sum(lengths)
    assert M != x.shape[0] * x.shape[2]
    for k, v in o.buffers.items():
        assert rel_err(dict(m.named_buffers())[k].cpu().numpy(), v.numpy()) < O.BARS["out"], k
    m.eval()
    with torch.no_grad():
        y = m(dev(x), lengths=list(lengths))
        assert torch.equal(m.forward_padded(dev(x), lengths), y)  # eval(): forward_padded is forward(lengths=)
    assert float(padded(y, lengths).abs().max()) == 0.0
    # the eval restatement on the model's own state_dict, each utterance alone (the eval ragged path's definition)
    ev = TransformerOracle({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()})
    for b, n in enumerate(lengths):
        assert rel_err(y[b:b + 1, :, :n].cpu().numpy(), ev.forward(x[b:b + 1, :, :n]).numpy()) < O.BARS["out"], b


# ------------------------------------------------------------------------------------------------ 6
def pad_config():
    c = R.STEPS3
    return dict(steps_config(R.ragged_case(R.STEPS3_CASE)[0]), package_mode="pad_masked", generator_optimizer_params=dict(lr=c["lr"]),
                generator_grad_norm=c["grad_norm"], generator_scheduler_params=dict(step_size=c["step_size"], gamma=c["gamma"]),
                lambda_aux=c["lambda_aux"], train_max_steps=c["n"], discriminator_train_start_steps=c["n"])


def pad_batch(step):
    x, t, lengths = R.steps3_batch(step)
    return {"x": torch.from_numpy(x), "y": torch.from_numpy(t), "lengths": torch.tensor(lengths, dtype=torch.int32)}


def test_three_pad_masked_steps_through_the_trainer():
    params, sd, _, _, _ = R.ragged_case(R.STEPS3_CASE)
    tr = InversionTrainer(pad_config(), torch.device("cuda:0"))
    tr.G.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    tr.G.set_dropout_seed(O.DROPOUT_SEED)
    assert tr.optimizer["generator"].defaults.get("fused") is True
    before = int(tr.G.conv_blocks[0].bn1.num_batches_tracked)
    losses = [float(tr.train_step(pad_batch(s))["train/generator_loss"]) for s in range(R.STEPS3["n"])]
    # the same three steps written out: forward_padded, masked_l1_loss, clip, Adam, scheduler
    m = build(params, sd)
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
    ref, _ = R.run_steps3(torch.float64)
    errs = [abs(a - b) / abs(b) for a, b in zip(losses, ref)]
    print("losses", losses, "by hand", hand, "deviation from the float64 restatement", errs)
    assert max(abs(a - b) / abs(b) for a, b in zip(losses, hand)) < R.STEPS3_LOSS_BAR
    assert hand == losses  # (the same kernels in the same order: in fact bitwise)
    for (k, va), vb in zip(tr.G.state_dict().items(), m.state_dict().values()):
        assert torch.equal(va, vb), k
    assert max(errs) < R.STEPS3_LOSS_BAR
    assert tr.steps == R.STEPS3["n"] and int(tr.G.conv_blocks[0].bn1.num_batches_tracked) == before + R.STEPS3["n"]


# ------------------------------------------------------------------------------------------------ 7
def test_train_cli_in_pad_masked_mode_with_a_dev_set_then_decode(tmp_path):
    from articulatory_amd.bin import decode as D
    from articulatory_amd.bin import train as T

    cfg = dict(generator_type="Transformer", dataset_mode="a2m", format="npy", generator_params=dict(O.BASE, dropout=0.2),
               generator_optimizer_type="Adam", generator_optimizer_params=dict(lr=1e-3), generator_grad_norm=10, generator_scheduler_type="StepLR",
               generator_scheduler_params=dict(step_size=1000, gamma=0.5), use_mel_loss=True, lambda_aux=1.0, batch_size=4, batch_max_steps=8,
               hop_size=1, aux_context_window=1, train_max_steps=3, discriminator_train_start_steps=3, log_interval_steps=1, eval_interval_steps=2,
               package_mode="pad_masked", pad_bucket_batches=2, pad_max_frames=30)
    (tmp_path / "config.yml").write_text(yaml.safe_dump(cfg))
    rng = np.random.default_rng(0)
    lines = {"feats": [], "mel": []}
    for u, n in (("a", 50), ("b", 7), ("c", 1)):
        np.save(tmp_path / f"{u}-feats.npy", rng.standard_normal((n, 12)).astype(np.float32))
        np.save(tmp_path / f"{u}-mel.npy", rng.standard_normal((n, 8)).astype(np.float32))
        lines["feats"].append(f"{u} {tmp_path / (u + '-feats.npy')}")
        lines["mel"].append(f"{u} {tmp_path / (u + '-mel.npy')}")
    (tmp_path / "dev_feats.scp").write_text("\n".join(lines["feats"]) + "\n")
    (tmp_path / "dev_mel.scp").write_text("\n".join(lines["mel"]) + "\n")
    T.main(["--config", str(tmp_path / "config.yml"), "--outdir", str(tmp_path), "--synthetic", "12", "--max-steps", "3", "--verbose", "0",
            "--dev-feats-scp", str(tmp_path / "dev_feats.scp"), "--dev-audio-scp", str(tmp_path / "dev_mel.scp")])
    ck = tmp_path / "checkpoint-3steps.pkl"
    state = torch.load(ck, map_location="cpu")
    assert state["steps"] == 3 and int(state["model"]["generator"]["conv_blocks.0.bn1.num_batches_tracked"]) == 2  # (the reference trains from step 1 on)
    Transformer(**cfg["generator_params"]).load_state_dict(state["model"]["generator"], strict=True)
    best = torch.load(tmp_path / "best_mel_ckpt.pkl", map_location="cpu")
    assert best["steps"] == 2 and (tmp_path / "best_mel_step.txt").read_text().strip() == "2"
    dump = tmp_path / "dump"
    dump.mkdir()
    for u, n in (("a", 50), ("b", 7)):
        np.save(dump / f"{u}-feats.npy", rng.standard_normal((n, 12)).astype(np.float32))
    D.main(["--dumpdir", str(dump), "--outdir", str(tmp_path / "mel"), "--checkpoint", str(ck), "--batch-size", "2", "--verbose", "0"])
    for u, n in (("a", 50), ("b", 7)):
        y = np.load(tmp_path / "mel" / f"{u}_gen.npy")
        assert y.shape == (n, 8) and np.isfinite(y).all()


# ------------------------------------------------------------------------------------------------ 8
def test_refusals_on_the_device():
    params, sd, _, _, _ = R.ragged_case("mixed")
    m = build(params, sd)
    x = torch.zeros(2, 12, 5, device="cuda:0")
    before = (m._calls, int(m.conv_blocks[0].bn1.num_batches_tracked))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m.forward_padded(x, [1, 0])
    with pytest.raises(RuntimeError, match=r"lengths must lie in \[0, 5\]"):
        m.forward_padded(x, [5, 6])
    with pytest.raises(RuntimeError, match=r"lengths must lie in \[0, 5\]"):
        m.forward_padded(x, [5, -1])
    with pytest.raises(RuntimeError, match="lengths has 3 entries for a batch of 2"):
        m.forward_padded(x, [5, 3, 1])
    with pytest.raises(RuntimeError, match="needs lengths"):
        m.forward_padded(x, None)
    with pytest.raises(NotImplementedError, match=r"ragged training.*forward_padded"):
        m(x, lengths=[5, 3])
    assert (m._calls, int(m.conv_blocks[0].bn1.num_batches_tracked)) == before  # a refused call draws no mask and tracks no batch
    # the C entry point checks the host lengths itself, before anything is enqueued
    m._native_handle(train=True)
    lib, h = m._lib, m._handle
    out, stats = torch.zeros(2, 8, 5, device="cuda:0"), torch.zeros(7, 2, 128, device="cuda:0")
    ws, ws_ptr, ws_bytes = owned(lib.hificar_xfmr_train_workspace_bytes(h, 2, 5), 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for bad in ([1, 0], [5, 6], [-1, 5]):
        host = torch.tensor(bad, dtype=torch.int32)
        on_dev = host.to("cuda:0")
        rc = lib.hificar_xfmr_forward_train_ragged(h, x.data_ptr(), on_dev.data_ptr(), host.data_ptr(), out.data_ptr(), stats.data_ptr(), 2, 5, 0.2, 1, 0,
                                                   None, 0, ws_ptr, ws_bytes, stream)
        assert rc == -1, bad  # HIFICAR_E_INVALID
    rc = lib.hificar_xfmr_forward_train_ragged(h, x.data_ptr(), on_dev.data_ptr(), None, out.data_ptr(), stats.data_ptr(), 2, 5, 0.2, 1, 0, None, 0, ws_ptr,
                                               ws_bytes, None)
    assert rc == -1 and b"lengths_host" in lib.hificar_last_error()
    # a workspace of the dense size minus one byte is refused, and the ragged form needs no more than the dense one reports
    host = torch.tensor([5, 3], dtype=torch.int32)
    on_dev = host.to("cuda:0")
    need = lib.hificar_xfmr_train_workspace_bytes(h, 2, 5)
    rc = lib.hificar_xfmr_forward_train_ragged(h, x.data_ptr(), on_dev.data_ptr(), host.data_ptr(), out.data_ptr(), stats.data_ptr(), 2, 5, 0.2, 1, 0, None, 0,
                                               ws_ptr, need - 1, stream)
    assert rc == -4  # HIFICAR_E_WORKSPACE
    torch.cuda.synchronize()
