"""Training the ``Transformer`` feature model natively on a MI355X: the train()-mode forward (batch-statistics BatchNorm, dropout) and the
backward pass through ``hificar_xfmr_forward_train`` / ``hificar_xfmr_backward``, against the golden vectors of the REAL reference class in
train() mode (tools/make_golden_transformer_train.py; dropout 0) and against the float64 restatement tests/transformer_train_oracle.py (the
package's own dropout masks).  ``pytest -m gpu``.

Bars (transformer_train_oracle.BARS, the BiGRU training suite's): output, batch statistics and running buffers 2e-5 of the tensor's max, the
loss 1e-5 relative, dx and every gradient 2e-4 of the tensor's max (a conv bias in front of a batch norm, whose gradient is mathematically
zero: of its conv weight's).  tests/test_transformer_train_host.py admits every shape here: the restatement's own float32 run stays within
half of each bar against its float64 run.
"""

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

import transformer_train_oracle as O
from conftest import GOLDEN, rel_err
from test_transformer_train_host import golden_errors
from transformer_oracle import TransformerOracle
from articulatory_amd.bin.train import InversionTrainer
from articulatory_amd.models import Transformer

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def build(name, seed=O.DROPOUT_SEED, shapes=None):
    """The model of an entry of ``shapes`` (transformer_train_oracle.SHAPES, or its EDGE_SHAPES) on the device in train() mode, and the
    entry's batch."""
    params, sd, x, t = O.case(name, shapes=shapes)
    m = Transformer(**params)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to("cuda:0").train()
    m.set_dropout_seed(seed)
    return m, x, t


def step(m, x, t, need_dx=True, gates=None):
    """One forward + backward of the L1 loss on the device, in the restatement's result layout.  ``gates``: a dict that receives which side
    of every ReLU the device took (hificar_xfmr_debug_tap), in the restatement's shapes."""
    for p in m.parameters():
        p.grad = None
    xt = dev(x).requires_grad_(need_dx)
    bufs = {}
    if gates is not None:
        B, _, T = x.shape
        m._native_handle(train=True)
        for name in O.relu_names(m._params):
            bufs[name] = torch.zeros((B, T, 3072 if name.endswith("hidden") else m._params["hidden_dim"]), dtype=torch.float32, device="cuda:0")
            m.debug_tap(name, bufs[name])
    y = m(xt)
    if gates is not None:
        m.debug_tap(None)
        for name, buf in bufs.items():
            gates[name] = (buf > 0).cpu() if name.endswith("hidden") else (buf > 0).transpose(1, 2).cpu()
    loss = F.l1_loss(y, dev(t))
    loss.backward()
    return dict(out=y.detach(), loss=loss.detach(), dx=xt.grad, grads={k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None},
                stats=m._last_stats.clone(), running={k: v.detach().clone() for k, v in m.named_buffers() if k.endswith(("running_mean", "running_var"))})


def reference(name, gates, shapes=None, device="cpu"):
    """The float64 restatement's step on a shape, every ReLU taken on the side the device took it (TransformerTrainOracle explains why);
    a gate may differ from the float64 run's own only where the ReLU's input is within GATE_GAP (the output bar) of zero.  ``device``: where
    the restatement (stock PyTorch in float64) runs."""
    ref = O.restatement(name, torch.float64, device=device, gates=gates, shapes=shapes)
    print(f"  {name}: {ref['gate_flips']} ReLU(s) on the other side than float64's own, the farthest {ref['gate_gap']:.3g} of max |x| from zero")
    assert ref["gate_gap"] < O.GATE_GAP
    return ref


def assert_within(errs, what):
    for k, (e, bar) in sorted(errs.items(), key=lambda kv: -kv[1][0] / kv[1][1])[:5]:
        print(f"  {what} {k}: {e:.3g} (bar {bar:g})")
    bad = {k: e for k, (e, bar) in errs.items() if not e < bar}
    assert not bad, (what, bad)


@pytest.mark.parametrize("name", list(O.SHAPES))
def test_step_against_the_restatement(name):
    m, x, t = build(name)
    before = [int(bn.num_batches_tracked) for bn in m._batch_norms()]  # (the synthetic state_dict's counters are not zero)
    gates = {}
    got = step(m, x, t, gates=gates)
    B, T = O.SHAPES[name][1:3]
    assert got["out"].shape == (B, 8, T) and got["out"].dtype == torch.float32
    assert_within(O.errors(got, reference(name, gates)), name)
    assert [int(bn.num_batches_tracked) for bn in m._batch_norms()] == [n + 1 for n in before] and m._calls == 1
    assert "libhificar.so" in open("/proc/self/maps").read()


def test_golden_case_of_the_reference_class():
    """Dropout 0 against the real class; its tables get no gradient there (padded under no_grad), which ``train_relative_positions = False``
    reproduces; the package's own table gradient is held to the restatement in test_step_against_the_restatement.  Where the device took a
    ReLU on the other side than float64 does (see ``reference``), the class's stored gradients are moved by what those gates change in the
    float64 restatement, which equals the class to rounding: nothing when no gate differs."""
    gold = np.load(os.path.join(GOLDEN, "gold_transformer_train.npz"))
    m, x, t = build(O.GOLD_CASE)
    m.train_relative_positions = False
    gates = {}
    got = step(m, x, t, gates=gates)
    nograd = set(gold[f"{O.GOLD_CASE}_nograd"].tolist())
    for k, p in m.named_parameters():
        assert (p.grad is None) == (k in nograd), k
    ref = reference(O.GOLD_CASE, gates)
    got["grads"] = {k: p.grad.detach().cpu().double() for k, p in m.named_parameters() if p.grad is not None}
    got["dx"] = got["dx"].cpu().double()
    if ref["gate_flips"]:
        own = O.restatement(O.GOLD_CASE, torch.float64)
        got["dx"] = got["dx"] - (ref["dx"] - own["dx"])
        got["grads"] = {k: g - (ref["grads"][k] - own["grads"][k]) for k, g in got["grads"].items()}
    assert_within(golden_errors(gold, O.GOLD_CASE, got), "golden")
    assert int(m.conv_blocks[0].bn1.num_batches_tracked) == int(gold[f"{O.GOLD_CASE}_num_batches_tracked"])


def steps_config(params):
    c = O.STEPS
    return dict(generator_type="Transformer", dataset_mode="a2m", generator_params=dict(params), generator_optimizer_type="Adam",
                generator_optimizer_params=dict(lr=c["lr"]), generator_grad_norm=c["grad_norm"], generator_scheduler_type="StepLR",
                generator_scheduler_params=dict(step_size=c["step_size"], gamma=c["gamma"]), lambda_aux=c["lambda_aux"], use_mel_loss=True,
                generator_train_start_steps=-1, train_max_steps=c["n"], discriminator_train_start_steps=c["n"])


def make_trainer():
    params, sd, _, _ = O.case(O.STEPS_CASE)
    tr = InversionTrainer(steps_config(params), torch.device("cuda:0"))
    tr.G.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    tr.G.set_dropout_seed(O.DROPOUT_SEED)
    return tr


def batch_of(s):
    _, _, x, t = O.case(O.STEPS_CASE, O.STEPS_FIRST + s)
    return {"x": torch.from_numpy(x), "y": torch.from_numpy(t)}


def test_five_steps_through_the_trainer_then_eval(tmp_path):
    """InversionTrainer.train_step with fused Adam and the device-side parameter refresh against the restatement's five steps: the losses at
    1e-4 (the BiGRU suite's bar for its five-step run; the restatement's own float32 run: 1.6e-6).  The final parameters are printed, not
    asserted: Adam's lr g / (|g| + eps) moves an element whose gradient is rounding noise by a noise-dependent share of lr, and the
    restatement's own float32 run ends 4e-3 of a tensor's max away from its float64 run (linear1.weight), twenty times the gradient bar —
    no seed or start batch changes that.  What the parameters became is checked where it is well conditioned: the eval-mode forward of the
    trained model against the eval restatement on the trained model's own state_dict, at the eval path's bar (2e-5), which also shows that
    the eval path sees the updated weights and running statistics; and a checkpoint round trip continues bitwise."""
    tr = make_trainer()
    assert tr.optimizer["generator"].defaults.get("fused") is True
    before = [int(bn.num_batches_tracked) for bn in tr.G._batch_norms()]
    losses = [float(tr.train_step(batch_of(s))["train/generator_loss"]) for s in range(O.STEPS["n"])]
    ref_losses, ref_final = O.five_steps(torch.float64)
    e_loss, worst = O.five_step_errors(losses, dict(tr.G.state_dict()), ref_losses, ref_final)
    print("losses", losses, "deviation", e_loss, "worst final tensor", max(worst, key=worst.get), max(worst.values()))
    assert e_loss < 1e-4
    assert tr.steps == O.STEPS["n"] and tr.G._calls == O.STEPS["n"]
    assert [int(bn.num_batches_tracked) for bn in tr.G._batch_norms()] == [n + O.STEPS["n"] for n in before]
    # eval after training: the folds are rebuilt from the updated parameters and running statistics on the device
    x = O.case(O.STEPS_CASE, 99)[2]
    tr.G.eval()
    y = tr.G(dev(x))
    sd = {k: v.detach().cpu().numpy() for k, v in tr.G.state_dict().items()}
    assert rel_err(y.cpu().numpy(), TransformerOracle(sd).forward(x).numpy()) < 2e-5
    fresh = Transformer(**O.case(O.STEPS_CASE)[0])
    fresh.load_state_dict(tr.G.state_dict(), strict=True)
    assert torch.equal(fresh.eval().to("cuda:0")(dev(x)), y)  # ... and equal what a handle built from the host copy computes
    tr.G.train()
    # checkpoint round trip: reference layout, strict load, and the next step is bitwise the unbroken run's
    path = str(tmp_path / "ck.pkl")
    tr.save_checkpoint(path)
    state = torch.load(path, map_location="cpu")
    assert set(state) >= {"model", "optimizer", "scheduler", "steps", "epochs"} and set(state["model"]) == {"generator"}
    tr2 = InversionTrainer(steps_config(O.case(O.STEPS_CASE)[0]), torch.device("cuda:0"))
    tr2.load_checkpoint(path)
    a = float(tr.train_step(batch_of(5))["train/generator_loss"])
    b = float(tr2.train_step(batch_of(5))["train/generator_loss"])
    assert a == b
    assert all(torch.equal(p, q) for p, q in zip(tr.G.state_dict().values(), tr2.G.state_dict().values()))


def test_deterministic_new_masks_streams_dirty_scratch_and_dx_on_request():
    name = "t65"  # p = 0.5
    m, x, t = build(name)
    a = step(m, x, t)
    # a second forward draws new masks (the generator's offset advanced)
    with torch.no_grad():
        y2 = m(dev(x))
    assert m._calls == 2 and not torch.equal(y2, a["out"])
    # the same seed and offset again: bitwise, with the workspace and a (recycled) tape full of NaNs, on a non-default stream, and without
    # grad mode the same output through the tape-less form
    m2, _, _ = build(name)
    m2._native_handle(train=True)
    m2._train_workspace(2, 65)
    ws = m2._train_ws_buf
    ws[: ws.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
    junk = torch.full((int(m2._lib.hificar_xfmr_tape_bytes(m2._handle, 2, 65)) // 4 + 64,), float("nan"), device="cuda:0")
    del junk  # (the caching allocator hands these bytes to the next tape)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        b = step(m2, x, t, need_dx=False)
    s.synchronize()
    assert b["dx"] is None
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["loss"], b["loss"]) and torch.equal(a["stats"], b["stats"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    m3, _, _ = build(name)
    with torch.no_grad():
        y3 = m3(dev(x))
    assert torch.equal(y3, a["out"])
    assert torch.equal(m3.conv_blocks[0].bn1.running_var, b["running"]["conv_blocks.0.bn1.running_var"])


def test_refusals_on_the_device():
    """forward(lengths=...) in train() mode stays refused now that ragged training exists: it is asked for by name, and the refusal names
    the way in (forward_padded; tests/test_gpu_transformer_ragged.py holds that call's own refusals)."""
    m, x, t = build("t2")
    before = (m._calls, int(m.conv_blocks[0].bn1.num_batches_tracked))
    with pytest.raises(NotImplementedError, match=r"forward\(lengths=\.\.\.\) in train\(\) mode is refused: ragged training.*forward_padded\(x, lengths\)"):
        m(dev(x), lengths=[2, 1])
    assert (m._calls, int(m.conv_blocks[0].bn1.num_batches_tracked)) == before  # a refused call draws no mask and tracks no batch
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(dev(x[:1, :, :1]))


def test_train_cli_on_synthetic_pairs_then_decode(tmp_path):
    """``python -m articulatory_amd.bin.train`` with a Transformer config trains a few steps on synthetic pairs; the checkpoint it writes is
    decoded by ``articulatory_amd.bin.decode`` in ``a2m`` mode."""
    from articulatory_amd.bin import decode as D
    from articulatory_amd.bin import train as T

    cfg = dict(generator_type="Transformer", dataset_mode="a2m", format="npy", generator_params=dict(O.BASE, dropout=0.2),
               generator_optimizer_type="Adam", generator_optimizer_params=dict(lr=1e-3), generator_grad_norm=10, generator_scheduler_type="StepLR",
               generator_scheduler_params=dict(step_size=1000, gamma=0.5), use_mel_loss=True, lambda_aux=1.0, batch_size=2, batch_max_steps=40,
               hop_size=1, aux_context_window=0, train_max_steps=3, discriminator_train_start_steps=3, log_interval_steps=1)
    (tmp_path / "config.yml").write_text(yaml.safe_dump(cfg))
    T.main(["--config", str(tmp_path / "config.yml"), "--outdir", str(tmp_path), "--synthetic", "8", "--verbose", "0"])
    ck = tmp_path / "checkpoint-3steps.pkl"
    state = torch.load(ck, map_location="cpu")
    assert state["steps"] == 3 and int(state["model"]["generator"]["conv_blocks.0.bn1.num_batches_tracked"]) == 2  # (a fresh model; the reference trains from step 1 on)
    dump = tmp_path / "dump"
    dump.mkdir()
    rng = np.random.default_rng(0)
    for u, n in (("a", 50), ("b", 7)):
        np.save(dump / f"{u}-feats.npy", rng.standard_normal((n, 12)).astype(np.float32))
    D.main(["--dumpdir", str(dump), "--outdir", str(tmp_path / "mel"), "--checkpoint", str(ck), "--batch-size", "2", "--verbose", "0"])
    for u, n in (("a", 50), ("b", 7)):
        y = np.load(tmp_path / "mel" / f"{u}_gen.npy")
        assert y.shape == (n, 8) and np.isfinite(y).all()
