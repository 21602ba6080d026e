"""CPU restatement of the BiGRU training step on a RAGGED batch of whole utterances (``BiGRU.forward_padded`` + ``masked_l1_loss``), built on
tests/bigru_train_oracle.py: ``pack_padded_sequence(enforce_sorted=False)`` through the same two ``nn.GRU`` modules (empty sequences left
out), the package's dropout masks on the PADDED (B, T, C) tensors, ``F.batch_norm(training=True)`` on the valid rows only, fc2 (+ tanh),
masked L1.  The semantics are this package's definition (the reference never masks).  float32 or float64.

Test infrastructure only: no file of the package imports it.
"""

from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import bigru_train_oracle as O
from articulatory_amd.utils.synth import synth_bigru_state_dict, uniform

# name -> (Cin, H, out, tanh, B, T, lengths, p, sequences per workgroup or None)
RAGGED_SHAPES = OrderedDict([
    ("mixed", (8, 64, 12, False, 4, 9, (9, 1, 0, 5), 0.3, None)),            # full, one frame, empty, partial
    ("tiles", (8, 64, 12, True, 3, 130, (130, 64, 65), 0.3, None)),          # a length on a head-tile edge and one past it
    ("ns2", (24, 128, 18, False, 3, 7, (7, 2, 5), 0.3, 2)),                  # an unequal pair in a tile, an odd tail
    ("h192", (24, 192, 18, False, 3, 7, (3, 7, 1), 0.3, 2)),
    ("h256", (24, 256, 18, False, 2, 40, (40, 17), 0.3, None)),              # the L2-streamed columns
    ("p0", (8, 64, 12, False, 3, 20, (20, 11, 3), 0.0, None)),
    ("one", (8, 64, 1, True, 2, 6, (6, 2), 0.5, None)),
    ("h256_ns2", (24, 256, 18, False, 3, 6, (6, 1, 4), 0.3, 2)),
    # the second trip of every grid-stride loop over masked rows (B T = 8580 rows)
    ("stride", (24, 64, 12, False, 66, 130, tuple((37 * b) % 131 for b in range(66)), 0.3, None)),
    ("b1", (8, 64, 12, False, 1, 5, (3,), 0.3, None)),
])
# (no seed was rejected by the admission rule of tests/test_bigru_ragged_host.py)
RAGGED_SEEDS = dict(mixed=7300, tiles=7301, ns2=7302, h192=7303, h256=7304, p0=7305, one=7306, h256_ns2=7310, stride=7311, b1=7312)


def ragged_case(name):
    """(model params, state_dict, x (B, in, T), target (B, out, T), lengths, sequences per workgroup or None) of a RAGGED_SHAPES entry;
    inputs and targets as bigru_train_oracle.edge_case draws them."""
    cin, H, out, tanh, B, T, lengths, p, ns = RAGGED_SHAPES[name]
    seed = RAGGED_SEEDS[name]
    params = dict(in_channels=cin, hidden_size=H, out_channels=out, use_tanh=tanh, dropout=p)
    x = uniform(seed, "x", (B, cin, T), -1.0, 1.0)
    t = uniform(seed, "t", (B, out, T), 4.0, 5.0) * np.where(uniform(seed, "s", (B, out, T), -1.0, 1.0) >= 0, 1.0, -1.0).astype(np.float32)
    assert len(lengths) == B and all(0 <= n <= T for n in lengths) and sum(lengths) >= 2
    return params, synth_bigru_state_dict(params, seed=seed), x, t, tuple(lengths), ns


def valid_mask(lengths, T):
    """(B, T) bool: frame t of sequence b is one of its own."""
    return torch.arange(T)[None, :] < torch.as_tensor(list(lengths), dtype=torch.long)[:, None]


def masked_l1(y, t, lengths):
    """sum over valid frames of |y - t| / (M C) for (B, C, T) tensors: the definition, written without the package."""
    v = valid_mask(lengths, y.shape[2])[:, None, :].to(y.dtype)
    return ((y - t).abs() * v).sum() / (float(sum(int(n) for n in lengths)) * y.shape[1])


class BiGRURaggedOracle(O.BiGRUTrainOracle):
    def _gru(self, g, y, lengths):
        """One bidirectional layer over each sequence's own frames: (B, T, C) -> (B, T, 2H), zeros on padded frames."""
        B, T, _ = y.shape
        idx = torch.as_tensor([b for b, n in enumerate(lengths) if n > 0], dtype=torch.long)
        lens = torch.as_tensor([int(lengths[int(b)]) for b in idx], dtype=torch.long)
        packed = pack_padded_sequence(y.index_select(0, idx), lens, batch_first=True, enforce_sorted=False)
        out, _ = g(packed)
        out, _ = pad_packed_sequence(out, batch_first=True, total_length=T)
        return torch.zeros((B, T, out.shape[2]), dtype=y.dtype).index_copy(0, idx, out)

    def forward_padded(self, x, lengths, train=True):
        """x (B, in, T), lengths -> (B, out, T), zeros past a length.  train: masks of the padded tensors, batch statistics of the valid rows
        (the call advances the mask offset and the running statistics); else the eval-mode forward on the running statistics."""
        P = self.params
        y = (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).to(self.dtype).transpose(1, 2)
        B, T, _ = y.shape
        offset = self.calls
        if train:
            self.calls += 1
        for i, g in enumerate(self.grus):
            y = self._gru(g, y, lengths)
            if train:
                y = self._mask(i, y, offset)
        y = F.linear(y, P["fc1.0.weight"], P["fc1.0.bias"])
        if train:
            y = self._mask(2, y, offset)
        valid = valid_mask(lengths, T)
        rows = y[valid]  # (M, 128), in (b, t) order
        rows = F.batch_norm(rows, self.running_mean, self.running_var, P["bn.weight"], P["bn.bias"], training=train, momentum=0.1, eps=1e-5)
        if train:
            self.num_batches_tracked += 1
        rows = F.linear(rows, P[self.fc2 + ".weight"], P[self.fc2 + ".bias"])
        if self.use_tanh:
            rows = torch.tanh(rows)
        out = torch.zeros((B, T, rows.shape[1]), dtype=self.dtype).masked_scatter(valid[:, :, None], rows)
        return out.transpose(1, 2)

    def gru_outputs(self, x, lengths):
        """The first layer's outputs (B, T, 2H) without masks (for the test that a sequence of a ragged batch is that sequence alone)."""
        y = torch.as_tensor(np.asarray(x)).to(self.dtype).transpose(1, 2)
        return self._gru(self.grus[0], y, lengths)

    def loss_and_grads_padded(self, x, target, lengths, lambda_aux=1.0):
        """One forward + backward of the masked L1 loss: (y, loss, {key: grad}, dx)."""
        for v in self.params.values():
            v.grad = None
        xt = torch.as_tensor(np.asarray(x)).to(self.dtype).requires_grad_(True)
        y = self.forward_padded(xt, lengths)
        loss = masked_l1(y, torch.as_tensor(np.asarray(target)).to(self.dtype), lengths) * lambda_aux
        loss.backward()
        return y.detach(), loss.detach(), OrderedDict((k, v.grad.detach().clone()) for k, v in self.params.items()), xt.grad.detach()


def ragged_restatement(name, dtype):
    """One step of the restatement on a RAGGED_SHAPES entry: dict(y, loss, dx, running_mean, running_var, kink, grad.<key> ...); kink is
    taken over the valid frames."""
    params, sd, x, t, lengths, _ = ragged_case(name)
    o = BiGRURaggedOracle(sd, use_tanh=params["use_tanh"], dropout=params["dropout"], dtype=dtype)
    y, loss, grads, dx = o.loss_and_grads_padded(x, t, lengths)
    v = valid_mask(lengths, y.shape[2])[:, None, :].expand_as(y)
    res = dict(y=y, loss=loss, dx=dx, running_mean=o.running_mean, running_var=o.running_var,
               kink=float((y - torch.from_numpy(t).to(dtype)).abs()[v].min() / y.abs().max()))
    for k, g in grads.items():
        res["grad." + k] = g
    return res


# ------------------------------------------------------------------------------------------------
# three steps of the trainer on `pad` batches (tests/test_gpu_bigru_ragged.py): model of golden case c0, Adam, clipping, StepLR
# ------------------------------------------------------------------------------------------------
STEPS3 = dict(n=3, lr=1e-3, grad_norm=10.0, step_size=1, gamma=0.5, lambda_aux=1.0)
STEPS3_LENGTHS = ((37, 12, 25), (30, 37, 1), (5, 19, 37))  # per step: B 3, padded to T 37
STEPS3_LOSS_BAR = 1e-4      # the loss bar of test_gpu_bigru_train.py::test_five_steps_through_the_trainer
# the first batch number of case c0 from which the restatement's own float32 three steps stay within half the bar of its float64 steps
# (tests/test_bigru_ragged_host.py checks it); starts rejected by that rule: none
STEPS3_FIRST_BATCH = 0


def steps3_batch(step):
    x, t = O.case_batch("c0", STEPS3_FIRST_BATCH + step)
    return x, t, STEPS3_LENGTHS[step]


def run_steps3(dtype):
    """The losses of the three steps in ``dtype``, and the oracle after them."""
    params = O.case_params("c0")[0]
    o = BiGRURaggedOracle(O.case_state_dict("c0"), use_tanh=params["use_tanh"], dropout=params["dropout"], dtype=dtype)
    opt = torch.optim.Adam(list(o.params.values()), lr=STEPS3["lr"])
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=STEPS3["step_size"], gamma=STEPS3["gamma"])
    losses = []
    for s in range(STEPS3["n"]):
        x, t, lengths = steps3_batch(s)
        y = o.forward_padded(torch.as_tensor(x).to(dtype), lengths)
        loss = masked_l1(y, torch.as_tensor(t).to(dtype), lengths) * STEPS3["lambda_aux"]
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(o.params.values()), STEPS3["grad_norm"])
        opt.step()
        sched.step()
        losses.append(float(loss.detach()))
    return losses, o
