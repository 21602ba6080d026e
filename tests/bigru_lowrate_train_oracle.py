"""CPU restatement of the BiGRU training step on LOW-RATE inputs (``BiGRU.forward_lowrate_train``): tests/predict_ema_oracle.py's front end
(interpolation by ``source_index``, per-utterance z-score) written as a constant matrix per sequence, so that autograd carries the input's
gradient back through the interpolation, in front of tests/bigru_train_oracle.py (dense) / tests/bigru_ragged_oracle.py (ragged) — the step
those modules hold ``forward`` / ``forward_padded`` to, on the stretched input.  float32 or float64.  Also the numpy restatement of the
adjoint interpolation as the device forms it (a gather over one contiguous run of frames per low-rate frame).

Test infrastructure only: no file of the package imports it.
"""

from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import bigru_ragged_oracle as R
import bigru_train_oracle as O
import predict_ema_oracle as P
from articulatory_amd.utils.synth import synth_bigru_state_dict, uniform

# name -> (Cin, H, out, tanh, B, factor, Tl, low-rate lengths or None, p, sequences per workgroup or None, zscore)
LOW_SHAPES = OrderedDict([
    ("a16", (24, 64, 12, False, 3, 4, 16, None, 0.3, None, False)),      # T 64: the head's 64-frame tile exactly full
    ("a17", (24, 64, 12, False, 3, 4, 17, None, 0.3, None, False)),      # T 68: ... with a tail
    ("a33", (24, 64, 12, False, 3, 4, 33, None, 0.3, None, False)),      # T 132: three tiles deep
    ("b_f3", (13, 64, 1, True, 2, 3, 43, None, 0.3, None, False)),       # an odd factor, T 129, one output row through tanh'
    ("b_f2_l1", (13, 64, 1, True, 2, 2, 1, None, 0.3, None, False)),     # one low-rate frame: repeated, its gradient the sum
    ("b_f2_l2", (13, 64, 1, True, 2, 2, 2, None, 0.3, None, False)),     # two: the first and the last frame's runs only
    ("b_f16", (13, 64, 1, True, 2, 16, 3, None, 0.3, None, False)),      # the largest factor
    ("c", (1024, 256, 18, False, 2, 4, 20, None, 0.3, None, False)),     # the published widths
    ("d", (24, 128, 12, False, 5, 4, 24, (24, 1, 0, 17, 9), 0.3, None, False)),   # ragged: full, one frame, empty, partial
    ("d_p0", (24, 128, 12, False, 5, 4, 24, (24, 1, 0, 17, 9), 0.0, None, False)),
    ("e", (24, 128, 12, False, 5, 4, 24, (24, 1, 0, 17, 9), 0.3, 2, False)),      # ... an unequal pair shares a sweep tile
    ("e_p0", (24, 128, 12, False, 5, 4, 24, (24, 1, 0, 17, 9), 0.0, 2, False)),
    ("z", (13, 64, 1, True, 2, 3, 43, None, 0.3, None, True)),           # case b_f3 z-scored (statistics as constants)
])
# (no seed was rejected by the admission rule of tests/test_bigru_lowrate_train_host.py)
LOW_SEEDS = {name: 7500 + i for i, name in enumerate(LOW_SHAPES)}
LOW_SEEDS["e"], LOW_SEEDS["e_p0"] = LOW_SEEDS["d"], LOW_SEEDS["d_p0"]  # case E is case D in another sweep tile
# the cases of tests/golden/gold_bigru_lowrate_train.npz (tools/make_golden_bigru_lowrate_train.py: the reference's own BiGRU in train() mode on
# F.interpolate'd input, float64): dense ones, the reference never masks
GOLD = ("a17", "b_f3", "b_f2_l1")


def low_case(name):
    """(model params, state_dict, x (B, in, Tl), target (B, out, f Tl), factor, low-rate lengths or None, sequences per workgroup or None,
    zscore) of a LOW_SHAPES entry; inputs and targets as bigru_train_oracle.edge_case draws them."""
    cin, H, out, tanh, B, f, Tl, lengths, p, ns, zs = LOW_SHAPES[name]
    seed = LOW_SEEDS[name]
    params = dict(in_channels=cin, hidden_size=H, out_channels=out, use_tanh=tanh, dropout=p)
    x = uniform(seed, "x", (B, cin, Tl), -1.0, 1.0)
    if zs:
        x = (3.0 * x + 0.5).astype(np.float32)  # a mean and a scale for the z-score to take out
    t = uniform(seed, "t", (B, out, f * Tl), 4.0, 5.0) * np.where(uniform(seed, "s", (B, out, f * Tl), -1.0, 1.0) >= 0, 1.0, -1.0).astype(np.float32)
    assert lengths is None or (len(lengths) == B and all(0 <= n <= Tl for n in lengths) and f * sum(lengths) >= 2)
    return params, synth_bigru_state_dict(params, seed=seed), x, t, f, lengths, ns, zs


def interp_matrix(f, l):
    """A (f l, l) float64: stretched = A @ frames, by predict_ema_oracle.source_index (rows sum to one)."""
    A = np.zeros((f * l, l))
    if l == 0:
        return A
    t = np.arange(f * l)
    i0, i1, lam = P.source_index(t, f, l)
    np.add.at(A, (t, i0), 1.0 - lam)
    np.add.at(A, (t, i1), lam)
    return A


def first_frame(j, f):
    """The first output frame whose source frame i0 (before the clamp at l - 1) is j: 2 t + 1 - f >= 2 f j."""
    return 0 if j <= 0 else f * j + f // 2


def adjoint_gather(d, f, l):
    """The device's adjoint interpolation restated: d (f l, N) -> (l, N).  Low-rate frame i sums, in ascending t over ONE contiguous run
    — from the first frame whose i0 is i - 1 to the first whose i0 is i + 1 (the last frame: to f l) — (1 - lam) d[t] where i0 = i and
    lam d[t] where i1 = i != i0.  Also returns, per output frame, how often it was used as an i0-frame and as an i1-frame."""
    d = np.asarray(d, dtype=np.float64)
    out = np.zeros((l, d.shape[1]))
    used0, used1 = np.zeros(f * l, dtype=int), np.zeros(f * l, dtype=int)
    for i in range(l):
        end = f * l if i == l - 1 else first_frame(i + 1, f)
        for t in range(first_frame(i - 1, f), end):
            i0, i1, lam = (v.item() for v in P.source_index(np.array(t), f, l))
            if i0 == i:
                out[i] += (1.0 - lam) * d[t]
                used0[t] += 1
            else:
                assert i1 == i and i0 == i - 1, (f, l, i, t)
                out[i] += lam * d[t]
                used1[t] += 1
    return out, used0, used1


def stretch(x, f, lengths, zscore, dtype):
    """x (B, C, Tl) torch tensor (may require grad) -> (B, C, f Tl) in ``dtype``: every sequence by its own low-rate length (None: Tl), zeros
    past f lengths[b]; padded frames of x are not read.  The z-score's statistics are constants (computed in float64 from the values)."""
    B, C, Tl = x.shape
    rows = []
    for b in range(B):
        l = Tl if lengths is None else int(lengths[b])
        u = x[b, :, :l].to(dtype)
        if zscore and l > 0:
            v = u.detach().double().numpy()
            mu = v.sum() / v.size
            sd = np.sqrt(((v - mu) ** 2).sum() / v.size)
            u = ((u.double() - mu) / sd).to(dtype)
        A = torch.from_numpy(interp_matrix(f, l)).to(dtype)
        rows.append(torch.cat([u @ A.T, torch.zeros((C, f * (Tl - l)), dtype=dtype)], dim=1))
    return torch.stack(rows)


def low_restatement(name, dtype):
    """One step of the restatement on a LOW_SHAPES entry: dict(y, loss, dx (at the LOW rate, through the interpolation; None with zscore),
    running_mean, running_var, kink, grad.<key> ...)."""
    params, sd, x, t, f, lengths, _, zs = low_case(name)
    cls = O.BiGRUTrainOracle if lengths is None else R.BiGRURaggedOracle
    o = cls(sd, use_tanh=params["use_tanh"], dropout=params["dropout"], dtype=dtype)
    xl = torch.from_numpy(x).to(dtype).requires_grad_(not zs)
    xh = stretch(xl, f, lengths, zs, dtype)
    tt = torch.from_numpy(t).to(dtype)
    if lengths is None:
        y = o.forward(xh)
        loss = F.l1_loss(y, tt)
        valid = torch.ones_like(y, dtype=torch.bool)
    else:
        hi = [f * int(n) for n in lengths]
        y = o.forward_padded(xh, hi)
        loss = R.masked_l1(y, tt, hi)
        valid = R.valid_mask(hi, y.shape[2])[:, None, :].expand_as(y)
    loss.backward()
    res = dict(y=y.detach(), loss=loss.detach(), dx=None if zs else xl.grad.detach(), running_mean=o.running_mean, running_var=o.running_var,
               kink=float((y.detach() - tt).abs()[valid].min() / y.detach().abs().max()))
    for k, v in o.params.items():
        res["grad." + k] = v.grad.detach().clone()
    return res
