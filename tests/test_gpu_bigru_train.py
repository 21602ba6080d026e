"""Training the ``BiGRU`` inversion model natively on a MI355X: the train()-mode forward (dropout, batch-statistics BatchNorm) and the backward
pass through ``hificar_bigru_forward_train`` / ``hificar_bigru_backward``, against golden vectors of the REAL reference class in train() mode
(tools/make_golden_bigru_train.py) and against the float64 CPU restatement tests/bigru_train_oracle.py.  ``pytest -m gpu``.

Bars: outputs and running statistics 2e-5 of the tensor's max (the exact-fp32 bar), the loss 1e-5 relative, gradients 2e-4 of the tensor's
scale (the bar of tests/test_gpu_train.py for exact-fp32 training kernels; a golden gradient's scale is stored with it: its own max, except
in the one case whose upstream gradients are exactly zero in float64 — the un-cancelled term's there, see the tool's docstring).
"""

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bigru_train_oracle as O
from bigru_oracle import BiGRUOracle
from conftest import GOLDEN, rel_err
from articulatory_amd.bin.train import InversionTrainer
from articulatory_amd.models import BiGRU
from articulatory_amd.utils.synth import synth_bigru_state_dict, uniform

pytestmark = pytest.mark.gpu
TOL_OUT, TOL_LOSS, TOL_GRAD = 2e-5, 1e-5, 2e-4


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "gold_bigru_train.npz"))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def build(params, sd, seed=O.DROPOUT_SEED):
    m = BiGRU(**params)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to("cuda:0").train()
    m.set_dropout_seed(seed)
    return m


def step(m, x, t, need_dx=True):
    """One forward + backward of the L1 loss on the device: (y, loss, {key: grad}, dx)."""
    for p in m.parameters():
        p.grad = None
    xt = dev(x).requires_grad_(need_dx)
    y = m(xt)
    loss = F.l1_loss(y, dev(t))
    loss.backward()
    return y.detach(), loss.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}, xt.grad


@pytest.mark.parametrize("tag", list(O.GOLD_CASES))
def test_golden_case(gold, tag):
    params, B, T, _ = O.case_params(tag)
    m = build(params, O.case_state_dict(tag))
    x, t = O.case_batch(tag)
    y, loss, grads, dx = step(m, x, t)
    assert y.shape == (B, params["out_channels"], T) and y.dtype == torch.float32
    e_y = rel_err(y.cpu().numpy(), gold[f"{tag}_y"])
    e_l = abs(float(loss) - float(gold[f"{tag}_loss"][0])) / abs(float(gold[f"{tag}_loss"][0]))
    print(f"{tag}: y {e_y:.3g}, loss {e_l:.3g}")
    worst = {"dx": O.deviation(gold, f"{tag}_dx", dx)}
    for k, g in grads.items():
        worst[k] = O.deviation(gold, f"{tag}_grad.{k}", g)
    for k, e in worst.items():
        print(f"  {tag} grad {k}: {e:.3g}")
    e_m = rel_err(m.bn.running_mean.cpu().numpy(), gold[f"{tag}_running_mean"])
    e_v = rel_err(m.bn.running_var.cpu().numpy(), gold[f"{tag}_running_var"])
    print(f"  {tag} running_mean {e_m:.3g}, running_var {e_v:.3g}")
    assert e_y < TOL_OUT and e_l < TOL_LOSS
    assert max(worst.values()) < TOL_GRAD, max(worst, key=worst.get)
    assert e_m < TOL_OUT and e_v < TOL_OUT
    assert int(m.bn.num_batches_tracked) == int(gold[f"{tag}_num_batches_tracked"])
    assert "libhificar.so" in open("/proc/self/maps").read()


def steps_config(params):
    c = O.STEPS
    return dict(generator_type="BiGRU", dataset_mode="art", generator_params=dict(params), generator_optimizer_type="Adam",
                generator_optimizer_params=dict(lr=c["lr"]), generator_grad_norm=c["grad_norm"], generator_scheduler_type="StepLR",
                generator_scheduler_params=dict(step_size=c["step_size"], gamma=c["gamma"]), lambda_aux=c["lambda_aux"], use_mel_loss=True,
                generator_train_start_steps=-1, train_max_steps=c["n"], discriminator_train_start_steps=c["n"])


def make_trainer(seed=O.DROPOUT_SEED):
    params = O.case_params("c0")[0]
    tr = InversionTrainer(steps_config(params), torch.device("cuda:0"))
    tr.G.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in O.case_state_dict("c0").items()}, strict=True)
    tr.G.set_dropout_seed(seed)
    return tr


def batch_of(step_no):
    x, t = O.case_batch("c0", step_no)
    return {"x": torch.from_numpy(x), "y": torch.from_numpy(t)}


def test_five_steps_through_the_trainer(gold):
    """InversionTrainer.train_step with fused Adam and the device-side parameter refresh, against the reference's own five steps.

    The run starts at batch 30 of case c0, not 0: Adam's first steps are lr g / (|g| + 1e-8), so an element whose gradient is within fp32
    noise of zero moves by a noise-dependent share of lr, and the reference's own fp32 run misses the admission bar (2e-5 of a final
    tensor's max against its float64 run) from batches 0 (gru2.weight_hh_l0 2.5e-5), 10 (gru1.weight_ih_l0_reverse 2.2e-5,
    gru2.weight_ih_l0_reverse 2.6e-5, fc1.0.weight 5.5e-5) and 20 (gru2.weight_ih_l0 2.2e-5), each by a few elements; from 30 it is within
    1.3e-5.  The fixture keeps the rejected starts (``steps_rejected``): isolated tensors just over the bar, no systematic gap."""
    tr = make_trainer()
    assert tr.optimizer["generator"].defaults.get("fused") is True
    first = int(gold["steps_first_batch"])
    losses = [float(tr.train_step(batch_of(first + s))["train/generator_loss"]) for s in range(O.STEPS["n"])]
    ref = gold["steps_losses"]
    errs = [abs(a - b) / abs(b) for a, b in zip(losses, ref)]
    print("losses", losses, "errs", errs)
    worst = {k: O.deviation(gold, "steps_final." + k, v) for k, v in tr.G.state_dict().items() if v.dtype.is_floating_point}
    for k, e in worst.items():
        print(f"  final {k}: {e:.3g}")
    assert max(errs) < 1e-4
    assert max(worst.values()) < TOL_GRAD, max(worst, key=worst.get)
    assert tr.steps == O.STEPS["n"] and int(tr.G.bn.num_batches_tracked) == int(gold["steps_num_batches_tracked"])


# the shapes where the kernels change form, against the float64 restatement: (Cin, H, out, B, T, p, sequences per workgroup or None)
SHAPES = {
    "h192": (24, 192, 18, 2, 16, 0.3, None),       # W_hh^T in registers + an LDS slab
    "h256": (24, 256, 18, 2, 16, 0.3, None),       # ... + a stream from L2
    "h256_ns2": (24, 256, 18, 2, 16, 0.3, 2),      # the two-sequence tile's smaller register share
    "wide_in": (1024, 256, 18, 2, 8, 0.3, None),   # a wide input GEMM and its weight gradient
    "b3": (8, 64, 12, 3, 4, 0.3, None),            # one sequence per workgroup
    "b3_ns2": (8, 64, 12, 3, 4, 0.3, 2),           # two per workgroup with an odd tail tile
    "b130": (8, 64, 12, 130, 4, 0.3, None),        # more sequences than half the chip's CUs: two per workgroup by choice
    "t1_h256": (24, 256, 18, 5, 1, 0.3, None),     # no recurrence at all
    "p0": (24, 64, 12, 3, 9, 0.0, None),           # p = 0: the identity, through batch statistics only
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_against_float64_restatement(name, monkeypatch):
    cin, H, out, B, T, p, ns = SHAPES[name]
    if ns is not None:
        monkeypatch.setenv("HIFICAR_BIGRU_NS", str(ns))
    params = dict(in_channels=cin, hidden_size=H, out_channels=out, use_tanh=False, dropout=p)
    seed = 7000 + sorted(SHAPES).index(name)
    sd = synth_bigru_state_dict(params, seed=seed)
    x = uniform(seed, "x", (B, cin, T), -1.0, 1.0)
    t = uniform(seed, "t", (B, out, T), 4.0, 5.0) * np.where(uniform(seed, "s", (B, out, T), -1.0, 1.0) >= 0, 1.0, -1.0).astype(np.float32)
    ref = O.BiGRUTrainOracle(sd, use_tanh=False, dropout=p, dtype=torch.float64)
    y64, l64, g64, dx64 = ref.loss_and_grads(x, t)
    assert float((y64 - torch.from_numpy(t).double()).abs().min()) > 1e-4 * float(y64.abs().max())  # kink-free
    m = build(params, sd)
    y, loss, grads, dx = step(m, x, t)
    e_y = rel_err(y.cpu().numpy(), y64.numpy())
    e_l = abs(float(loss) - float(l64)) / abs(float(l64))
    worst = {"dx": rel_err(dx.cpu().numpy(), dx64.numpy())}
    for k, g in grads.items():
        scale = g64["fc1.0.weight"].abs().max() if (k == "fc1.0.bias" and p == 0) else g64[k].abs().max()
        worst[k] = float((g.cpu().double() - g64[k]).abs().max() / scale)
    print(f"{name}: y {e_y:.3g}, loss {e_l:.3g}, worst grad {max(worst, key=worst.get)} {max(worst.values()):.3g}")
    e_m = rel_err(m.bn.running_mean.cpu().numpy(), ref.running_mean.numpy())
    e_v = rel_err(m.bn.running_var.cpu().numpy(), ref.running_var.numpy())
    assert e_y < TOL_OUT and e_l < TOL_LOSS
    assert max(worst.values()) < TOL_GRAD, max(worst, key=worst.get)
    assert e_m < TOL_OUT and e_v < TOL_OUT


def test_eval_after_training_is_the_eval_path_on_the_updated_statistics():
    params, _, _, _ = O.case_params("c0")
    m = build(params, O.case_state_dict("c0"))
    x, t = O.case_batch("c0")
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, fused=True)
    for _ in range(2):
        opt.zero_grad()
        F.l1_loss(m(dev(x)), dev(t)).backward()
        opt.step()
    m.eval()
    with torch.no_grad():
        y = m(dev(x))
    ref = BiGRUOracle({k: v.cpu().numpy() for k, v in m.state_dict().items()}, use_tanh=params["use_tanh"])
    assert rel_err(y.cpu().numpy(), ref.forward(x).numpy()) < TOL_OUT
    fresh = BiGRU(**params)  # ... and bit for bit what a model built from the same state_dict computes
    fresh.load_state_dict(m.state_dict(), strict=True)
    with torch.no_grad():
        assert torch.equal(fresh.to("cuda:0").eval()(dev(x)), y)


def test_bitwise_repeatable_and_a_second_forward_draws_a_new_mask():
    params, _, _, _ = O.case_params("c0")
    x, t = O.case_batch("c0")
    runs = []
    for _ in range(2):
        m = build(params, O.case_state_dict("c0"), seed=4242)
        y, loss, grads, dx = step(m, x, t)
        runs.append((y, grads, dx))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    with torch.no_grad():  # train() mode without grad: the same arithmetic, offset 1 -> another mask
        y2 = m(dev(x))
    assert not torch.equal(y2, runs[1][0])
    other = build(params, O.case_state_dict("c0"), seed=4243)
    with torch.no_grad():
        assert not torch.equal(other(dev(x)), runs[0][0])
    m.set_dropout_seed(4242)
    with torch.no_grad():
        assert torch.equal(m(dev(x)), runs[0][0])  # reseeded: offset 0 again (the running statistics do not enter a train() forward)


def test_non_default_stream_and_input_gradient_on_request():
    params, _, _, _ = O.case_params("c1")
    x, t = O.case_batch("c1")
    m = build(params, O.case_state_dict("c1"))
    y0, _, g0, dx0 = step(m, x, t)
    m2 = build(params, O.case_state_dict("c1"))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        y1, _, g1, dx1 = step(m2, x, t)
    s.synchronize()
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    m3 = build(params, O.case_state_dict("c1"))
    y2, _, g2, dx2 = step(m3, x, t, need_dx=False)
    assert dx2 is None and torch.equal(y2, y0)
    for k in g0:
        assert torch.equal(g0[k], g2[k]), k


def test_refusals_in_train_mode():
    params, _, _, _ = O.case_params("c0")
    m = build(params, O.case_state_dict("c0"))
    with pytest.raises(NotImplementedError, match="lengths"):
        m(torch.zeros(2, 24, 5, device="cuda:0"), lengths=[5, 3])
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(torch.zeros(1, 24, 1, device="cuda:0"))
    with pytest.raises(NotImplementedError, match="use_ar"):
        BiGRU(use_ar=True)
    with pytest.raises(NotImplementedError, match="use_spk_emb"):
        BiGRU(use_spk_emb=True)


def test_sizes_and_gradient_layout():
    params, _, _, _ = O.case_params("c0")
    m = build(params, O.case_state_dict("c0"))
    m(dev(O.case_batch("c0")[0]))
    lib, h = m._lib, m._handle
    assert 0 < lib.hificar_bigru_train_workspace_bytes(h, 3, 37) <= lib.hificar_bigru_train_workspace_bytes(h, 6, 370)
    assert 0 < lib.hificar_bigru_tape_bytes(h, 3, 37) < lib.hificar_bigru_tape_bytes(h, 6, 370)
    from articulatory_amd.models.bigru import _grad_layout

    layout = _grad_layout(m)
    named = dict(m.named_parameters())
    assert sorted(n for n, _, _ in layout) == sorted(named)  # the reference's state_dict keys, every trainable tensor once
    assert all(num == named[n].numel() for n, _, num in layout)
    spans = sorted((off, off + num) for _, off, num in layout)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= lib.hificar_bigru_grad_floats(h)


def test_train_cli_on_synthetic_pairs_then_decode(tmp_path):
    """``python -m articulatory_amd.bin.train`` with a BiGRU config trains a few steps on synthetic pairs; the checkpoint it writes is
    decoded by ``articulatory_amd.bin.decode`` in ``art`` mode."""
    import yaml

    from articulatory_amd.bin import decode as D
    from articulatory_amd.bin import train as T

    cfg = dict(generator_type="BiGRU", dataset_mode="art", format="npy", generator_params=dict(in_channels=24, hidden_size=64, out_channels=12, dropout=0.3),
               generator_optimizer_type="Adam", generator_optimizer_params=dict(lr=1e-3), generator_grad_norm=10, generator_scheduler_type="StepLR",
               generator_scheduler_params=dict(step_size=1000, gamma=0.5), use_mel_loss=True, lambda_aux=1.0, batch_size=4, batch_max_steps=32,
               hop_size=1, aux_context_window=2, train_max_steps=4, discriminator_train_start_steps=4, log_interval_steps=2)
    (tmp_path / "config.yml").write_text(yaml.safe_dump(cfg))
    T.main(["--config", str(tmp_path / "config.yml"), "--outdir", str(tmp_path), "--synthetic", "8", "--verbose", "0"])
    ck = tmp_path / "checkpoint-4steps.pkl"
    state = torch.load(ck, map_location="cpu")
    assert state["steps"] == 4 and int(state["model"]["generator"]["bn.num_batches_tracked"]) == 3  # (the reference trains from step 1 on)
    dump = tmp_path / "dump"
    dump.mkdir()
    rng = np.random.default_rng(0)
    for u, n in (("a", 50), ("b", 7)):
        np.save(dump / f"{u}-feats.npy", rng.standard_normal((n, 24)).astype(np.float32))
    D.main(["--dumpdir", str(dump), "--outdir", str(tmp_path / "ema"), "--checkpoint", str(ck), "--batch-size", "2", "--verbose", "0"])
    for u, n in (("a", 50), ("b", 7)):
        y = np.load(tmp_path / "ema" / f"{u}_gen.npy")
        assert y.shape == (n, 12) and np.isfinite(y).all()


def test_checkpoint_round_trip(tmp_path):
    a = make_trainer()
    for s in range(2):
        a.train_step(batch_of(s))
    path = str(tmp_path / "checkpoint-2steps.pkl")
    a.save_checkpoint(path)
    state = torch.load(path, map_location="cpu")
    assert set(state) >= {"model", "optimizer", "scheduler", "steps", "epochs"} and set(state["model"]) == {"generator"}
    BiGRU(**O.case_params("c0")[0]).load_state_dict(state["model"]["generator"], strict=True)
    b = InversionTrainer(steps_config(O.case_params("c0")[0]), torch.device("cuda:0"))
    b.load_checkpoint(path)
    assert b.steps == 2
    la = a.train_step(batch_of(2))["train/generator_loss"]
    lb = b.train_step(batch_of(2))["train/generator_loss"]
    assert torch.equal(la, lb)
    for (k, va), vb in zip(a.G.state_dict().items(), b.G.state_dict().values()):
        assert torch.equal(va, vb), k
