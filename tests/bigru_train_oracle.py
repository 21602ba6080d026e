"""CPU restatement of the BiGRU training step for the tests: the reference's train()-mode forward (pytorch_models.py:45-72) with torch's own
operators under autograd — torch.nn.GRU, F.linear, F.batch_norm(training=True), L1 loss — and the package's dropout masks
(``articulatory_amd.utils.synth.bigru_dropout_mask``) in place of nn.Dropout's.  float32 or float64.

Test infrastructure only: no file of the package imports it.
"""

from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from articulatory_amd.utils.synth import bigru_dropout_mask, synth_bigru_state_dict, uniform

# the cases of tests/golden/gold_bigru_train.npz (tools/make_golden_bigru_train.py): tag -> (in, H, out, tanh, B, T, p, seed)
GOLD_CASES = OrderedDict([
    ("c0", (24, 64, 12, False, 3, 37, 0.3, 6101)),
    ("c1", (13, 64, 12, True, 2, 50, 0.3, 6102)),
    ("c2", (24, 128, 12, False, 2, 20, 0.0, 6103)),
    ("c3", (24, 64, 1, False, 1, 2, 0.3, 6104)),
    ("c4", (24, 64, 12, False, 2, 1, 0.3, 6105)),
])
DROPOUT_SEED = 777          # every golden case: model seed of the mask generator, offset 0 for the first forward
STEPS = dict(n=5, lr=1e-3, grad_norm=10.0, step_size=1, gamma=0.5, lambda_aux=1.0)  # the five-step run on case c0 (StepLR halves lr every step)
FULL_LIMIT = 8192           # gradients up to this many elements are stored whole, larger ones packed (sum, |.|-sum, 64 samples)


# Shapes where the training kernels change form beyond what the golden cases and tests/test_gpu_bigru_train.py's SHAPES reach, against the
# float64 restatement: name -> (Cin, H, out, B, T, p, sequences per workgroup or None, tanh).  Each is admitted on the CPU first
# (tests/test_bigru_train_host.py): the restatement's own float32 run must be within half of every bar the device is held to.
EDGE_SHAPES = OrderedDict([
    ("t64", (8, 64, 12, 2, 64, 0.3, None, False)),          # the head's 64-frame tile exactly full
    ("t65", (8, 64, 12, 2, 65, 0.3, None, False)),          # ... a second tile of one frame
    ("t129", (8, 64, 12, 2, 129, 0.3, None, False)),        # ... three tiles, a one-frame tail
    ("t63_b1", (8, 64, 12, 1, 63, 0.3, None, False)),       # one short tile alone
    ("o32", (8, 64, 32, 2, 65, 0.3, None, False)),          # kBigruMaxOut output channels
    ("o32_tanh", (8, 64, 32, 2, 65, 0.3, None, True)),      # ... through tanh'
    ("o1_tanh", (8, 64, 1, 3, 70, 0.3, None, True)),        # one output row, tail tile
    ("h128_ns2", (24, 128, 18, 3, 5, 0.3, 2, False)),       # the <128, 2> sweeps, an odd tail tile of sequences
    ("h192_ns2", (24, 192, 18, 3, 5, 0.3, 2, False)),       # the <192, 2> sweeps
    ("t500", (24, 64, 12, 2, 500, 0.3, None, False)),       # the recurrence at the workload's length
    ("t300_h256", (24, 256, 18, 1, 300, 0.3, None, False)), # a long sweep with the L2-streamed columns of W_hh^T
    ("p05", (24, 64, 12, 3, 40, 0.5, None, False)),         # other dropout probabilities
    ("p09", (24, 64, 12, 3, 40, 0.9, None, False)),         # ... kept values scaled by 10
    # every grid-stride loop's second trip: B T = 8580 > 8192 rows, B T 2H = 4 392 960 > 4 194 304 elements; three head tiles with a 2-frame
    # tail, 269 rows per batch-norm lane.  B 66 stays at one sequence per workgroup (2 B <= the chip's 256 CUs), unlike SHAPES' b130.
    ("stride", (24, 256, 18, 66, 130, 0.3, None, False)),
])
EDGE_SEEDS = {name: 7100 + i for i, name in enumerate(EDGE_SHAPES)}
EDGE_BARS = dict(out=2e-5, loss=1e-5, grad=2e-4)  # the device's bars (tests/test_gpu_bigru_train.py: TOL_OUT, TOL_LOSS, TOL_GRAD)
KINK_MARGIN = 1e-4


def edge_case(name):
    """(model params, state_dict, x (B, in, T), target (B, out, T), sequences per workgroup or None) of an EDGE_SHAPES entry."""
    cin, H, out, B, T, p, ns, tanh = EDGE_SHAPES[name]
    seed = EDGE_SEEDS[name]
    params = dict(in_channels=cin, hidden_size=H, out_channels=out, use_tanh=tanh, dropout=p)
    x = uniform(seed, "x", (B, cin, T), -1.0, 1.0)
    # |y| is a few tenths without tanh and below 1 with it: targets in +-[4, 5] keep every |y - target| off the L1 kink
    t = uniform(seed, "t", (B, out, T), 4.0, 5.0) * np.where(uniform(seed, "s", (B, out, T), -1.0, 1.0) >= 0, 1.0, -1.0).astype(np.float32)
    return params, synth_bigru_state_dict(params, seed=seed), x, t, ns


def edge_restatement(name, dtype):
    """One step of the restatement on an EDGE_SHAPES entry: dict(y, loss, dx, running_mean, running_var, kink, grad.<key> ...)."""
    params, sd, x, t, _ = edge_case(name)
    o = BiGRUTrainOracle(sd, use_tanh=params["use_tanh"], dropout=params["dropout"], dtype=dtype)
    y, loss, grads, dx = o.loss_and_grads(x, t)
    res = dict(y=y, loss=loss, dx=dx, running_mean=o.running_mean, running_var=o.running_var,
               kink=float((y - torch.from_numpy(t).to(dtype)).abs().min() / y.abs().max()))
    for k, g in grads.items():
        res["grad." + k] = g
    return res


def edge_errors(got, ref, p):
    """{quantity: (deviation of ``got`` from the float64 results ``ref``, its bar)} for everything the device test checks: y and the running
    statistics relative to the tensor's max, the loss relative, every gradient relative to its own max (fc1.0.bias at p = 0, which is
    mathematically zero, to fc1.0.weight's)."""
    def rel(a, b):
        return float((torch.as_tensor(a).detach().cpu().double() - b).abs().max() / max(float(b.abs().max()), 1e-30))

    out = {"y": (rel(got["y"], ref["y"]), EDGE_BARS["out"]),
           "loss": (abs(float(got["loss"]) - float(ref["loss"])) / abs(float(ref["loss"])), EDGE_BARS["loss"]),
           "running_mean": (rel(got["running_mean"], ref["running_mean"]), EDGE_BARS["out"]),
           "running_var": (rel(got["running_var"], ref["running_var"]), EDGE_BARS["out"])}
    if got.get("dx") is not None:
        out["dx"] = (rel(got["dx"], ref["dx"]), EDGE_BARS["grad"])
    for k, r in ref.items():
        if not k.startswith("grad."):
            continue
        scale = ref["grad.fc1.0.weight"].abs().max() if (k == "grad.fc1.0.bias" and p == 0) else r.abs().max()
        out[k] = (float((torch.as_tensor(got[k]).detach().cpu().double() - r).abs().max() / scale), EDGE_BARS["grad"])
    return out


def case_params(tag):
    cin, H, out, tanh, B, T, p, seed = GOLD_CASES[tag]
    return dict(in_channels=cin, hidden_size=H, out_channels=out, use_tanh=tanh, dropout=p), B, T, seed


def case_batch(tag, step=0):
    """(x (B, in, T), target (B, out, T)) of a case, a pure function of (seed, step)."""
    params, B, T, seed = case_params(tag)
    x = uniform(seed, f"x.{step}", (B, params["in_channels"], T), -1.0, 1.0)
    # targets far from anything the model puts out (|y| is a few tenths): no |y_ - target| near the L1 kink
    t = uniform(seed, f"target.{step}", (B, params["out_channels"], T), 2.0, 3.0) * np.where(
        uniform(seed, f"sign.{step}", (B, params["out_channels"], T), -1.0, 1.0) >= 0, 1.0, -1.0).astype(np.float32)
    return x, t


def case_state_dict(tag):
    params, _, _, seed = case_params(tag)
    return synth_bigru_state_dict(params, seed=seed)


def pack(res, name, arr, scale=None, sumscale=None):
    """The fixture form of oracle.hificar_oracle.check_packed: the whole tensor when small, else sum / |.|-sum / 64 samples; ``scale``: what
    deviations of this tensor's elements are relative to (default: its own max), ``sumscale``: ... of its sums (default: its own |.|-sum,
    as check_packed).  The tool substitutes both only for a tensor that is rounding noise in the reference itself."""
    flat = np.asarray(arr, dtype=np.float64).reshape(-1)
    res[name + "::scale"] = np.array(float(np.abs(flat).max()) if scale is None else float(scale))
    res[name + "::sumscale"] = np.array(float(np.abs(flat).sum()) if sumscale is None else float(sumscale))
    if flat.size <= FULL_LIMIT:
        res[name + "::full"] = flat.astype(np.float32)
        return
    idx = np.linspace(0, flat.size - 1, 64).astype(np.int64)
    res[name + "::idx"] = idx
    res[name + "::vals"] = flat[idx].astype(np.float32)
    res[name + "::abssum"] = np.array(np.abs(flat).sum())
    res[name + "::sum"] = np.array(flat.sum())


def deviation(gold, name, arr):
    """Worst deviation of ``arr`` from the fixture entry ``name`` (written by ``pack``), relative to the entry's scale."""
    flat = np.asarray(arr.detach().cpu() if hasattr(arr, "detach") else arr, dtype=np.float64).reshape(-1)
    scale = max(float(gold[name + "::scale"]), 1e-30)
    if name + "::full" in gold:
        ref = gold[name + "::full"].astype(np.float64)
        assert ref.shape == flat.shape, (name, ref.shape, flat.shape)
        return float(np.abs(flat - ref).max() / scale)
    idx = gold[name + "::idx"]
    e1 = float(np.abs(flat[idx] - gold[name + "::vals"].astype(np.float64)).max() / scale)
    sumscale = max(float(gold[name + "::sumscale"]), 1e-30)  # check_packed's normalisation: the |.|-sum
    e2 = abs(float(np.abs(flat).sum()) - float(gold[name + "::abssum"])) / sumscale
    e3 = abs(float(flat.sum()) - float(gold[name + "::sum"])) / sumscale
    return max(e1, e2, e3)


class BiGRUTrainOracle:
    def __init__(self, state_dict, use_tanh=False, dropout=0.3, dtype=torch.float32, seed=DROPOUT_SEED):
        sd = {k: torch.as_tensor(np.asarray(v)) for k, v in state_dict.items()}
        self.dtype, self.use_tanh, self.p, self.seed, self.calls = dtype, use_tanh, float(dropout), seed, 0
        H = sd["gru1.weight_hh_l0"].shape[1]
        self.grus = []
        self.params = OrderedDict()  # reference state_dict key -> leaf tensor
        for name in ("gru1", "gru2"):
            g = torch.nn.GRU(input_size=sd[name + ".weight_ih_l0"].shape[1], hidden_size=H, num_layers=1, batch_first=True, bidirectional=True)
            g.load_state_dict({k[len(name) + 1:]: v for k, v in sd.items() if k.startswith(name + ".")}, strict=True)
            g = g.to(dtype).train()
            self.grus.append(g)
            for k, v in g.named_parameters():
                self.params[f"{name}.{k}"] = v
        fc2 = "fc2.0" if use_tanh else "fc2"
        for k in ("fc1.0.weight", "fc1.0.bias", "bn.weight", "bn.bias", fc2 + ".weight", fc2 + ".bias"):
            self.params[k] = sd[k].to(dtype).clone().requires_grad_(True)
        self.fc2 = fc2
        self.running_mean = sd["bn.running_mean"].to(dtype).clone()
        self.running_var = sd["bn.running_var"].to(dtype).clone()
        self.num_batches_tracked = int(sd["bn.num_batches_tracked"])

    def _mask(self, site, y, offset):
        if not self.p > 0:
            return y
        return y * torch.from_numpy(bigru_dropout_mask(self.seed, offset, site, tuple(y.shape), self.p)).to(self.dtype)

    def forward(self, x):
        """x (B, in, T) -> (B, out, T); advances the mask offset and the running statistics like a train()-mode call of the reference."""
        P = self.params
        offset = self.calls
        self.calls += 1
        y = (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).to(self.dtype).transpose(1, 2)
        for i, g in enumerate(self.grus):
            y, _ = g(y)
            y = self._mask(i, y, offset)
        y = self._mask(2, F.linear(y, P["fc1.0.weight"], P["fc1.0.bias"]), offset)
        y = F.batch_norm(y.transpose(1, 2), self.running_mean, self.running_var, P["bn.weight"], P["bn.bias"], training=True, momentum=0.1, eps=1e-5)
        self.num_batches_tracked += 1
        y = F.linear(y.transpose(1, 2), P[self.fc2 + ".weight"], P[self.fc2 + ".bias"])
        if self.use_tanh:
            y = torch.tanh(y)
        return y.transpose(1, 2)

    def loss_and_grads(self, x, target, lambda_aux=1.0):
        """One forward + backward of the L1 loss: (y, loss, {key: grad}, dx)."""
        for v in self.params.values():
            v.grad = None
        xt = torch.as_tensor(np.asarray(x)).to(self.dtype).requires_grad_(True)
        y = self.forward(xt)
        loss = F.l1_loss(y, torch.as_tensor(np.asarray(target)).to(self.dtype)) * lambda_aux
        loss.backward()
        return y.detach(), loss.detach(), OrderedDict((k, v.grad.detach().clone()) for k, v in self.params.items()), xt.grad.detach()


def run_steps(oracle, tag, cfg=STEPS):
    """The reference's generator step (train.py:268-383) cfg['n'] times on fresh batches of case ``tag``: Adam, gradient clipping, StepLR.
    Returns the losses; the oracle holds the final parameters and running statistics."""
    opt = torch.optim.Adam(list(oracle.params.values()), lr=cfg["lr"])
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=cfg["step_size"], gamma=cfg["gamma"])
    losses = []
    for step in range(cfg["n"]):
        x, t = case_batch(tag, step)
        y = oracle.forward(torch.as_tensor(x).to(oracle.dtype))
        loss = F.l1_loss(y, torch.as_tensor(t).to(oracle.dtype)) * cfg["lambda_aux"]
        opt.zero_grad()
        loss.backward()
        if cfg["grad_norm"] > 0:
            torch.nn.utils.clip_grad_norm_(list(oracle.params.values()), cfg["grad_norm"])
        opt.step()
        sched.step()
        losses.append(float(loss.detach()))
    return losses
