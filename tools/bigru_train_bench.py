#!/usr/bin/env python3
"""One training step of the BiGRU inversion model (forward in train() mode + L1 loss + backward + fused Adam) on the native kernels
(libhificar.so: hificar_bigru_forward_train / hificar_bigru_backward / hificar_bigru_set_parameters_device) next to the same step of the
same model from stock PyTorch-ROCm modules, on the same GPU in the same process.
   python tools/bigru_train_bench.py [--shapes full mfcc] [--batches 8 32] [--frames 200 500] [--window 0.3] [--out profiles/bigru_train.txt]

Shapes: full (1024, 256, 18) and mfcc (13, 256, 12, tanh).  Per (shape, B, T): device time from events, both warmed up, windows of at least
--window seconds alternated native / stock / native / stock (the two native windows run on unchanged code: their difference is the spread a
ratio has to exceed).  --limit seconds per step is checked from the events after each block of up to 16 steps and ends the run: it
cannot stop a step that hangs, so run the tool under an outer `timeout`.  Then one native step under hificar_profile_begin / hificar_profile_end:
time per kernel, the forward and the backward sweep's microseconds per step (kernel time / (2 layers * T)), and the tape / workspace bytes.
The stock model's dropout masks are torch's own (another random stream: the two steps are timed, not compared).
Prints one JSON line per case; --out also appends them to a file.

--ragged: one batch of whole utterances instead — the published shape (1024, 256, 18), B 32, padded to T 500, lengths uniform in 100 .. 500
from --seed — and three legs in alternated windows: the native ragged step (BiGRU.forward_padded + masked_l1_loss), the native dense step on
the same padded batch (every frame counted, as the reference's pad mode trains), and a stock PyTorch-ROCm ragged step (pack_padded_sequence
through nn.GRU, batch norm and L1 on the valid rows, the same optimizer).  Reports the padded-frame share and both native steps' kernel
and per-step sweep times.
   python tools/bigru_train_bench.py --ragged --out profiles/bigru_train_ragged.txt

--interp-factor N (> 1): training on low-rate inputs — the published shape (1024, 256, 18), x (B, 1024, T / N) for every B of --batches and
T of --frames (defaults: Tl 50 / 125 -> T 200 / 500 at N = 4), and two legs in windows alternated in one process: the low-rate step
(BiGRU.forward_lowrate_train: no stretched input, low-rate rows on the tape) against the materialised step (stock F.interpolate on the
device, then BiGRU.forward: what a user did before), the same loss and optimizer.  With --ragged: B 32, Tl 125, low-rate lengths uniform in
25 .. 125, forward_padded / masked_l1_loss on the materialised side (F.interpolate over the padded batch: timed, not compared — it clamps
at the padding, not at each utterance).  Reports both legs' windows, a verdict (a leg is called faster only when the gap exceeds the two
legs' window spreads added together, "not separated" otherwise), per-kernel times from the library's event profile and the tape and
workspace bytes of both legs.
   python tools/bigru_train_bench.py --interp-factor 4 --out profiles/bigru_train_lowrate.txt"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence  # noqa: E402

from articulatory_amd import _native  # noqa: E402
from articulatory_amd.losses import masked_l1_loss  # noqa: E402
from articulatory_amd.models import BiGRU  # noqa: E402
from articulatory_amd.utils.synth import synth_bigru_state_dict, uniform  # noqa: E402

SHAPES = {"full": dict(in_channels=1024, hidden_size=256, out_channels=18, use_tanh=False),
          "mfcc": dict(in_channels=13, hidden_size=256, out_channels=12, use_tanh=True)}
DROPOUT = 0.3


class StockBiGRU(torch.nn.Module):
    """The reference's module graph (pytorch_models.py:27-37, 62-72) from stock torch.nn modules, dropout included."""

    def __init__(self, in_channels, hidden_size, out_channels, use_tanh):
        super().__init__()
        self.gru1 = torch.nn.GRU(input_size=in_channels, hidden_size=hidden_size, num_layers=1, batch_first=True, bidirectional=True)
        self.dropout1 = torch.nn.Dropout(DROPOUT)
        self.gru2 = torch.nn.GRU(input_size=hidden_size * 2, hidden_size=hidden_size, num_layers=1, batch_first=True, bidirectional=True)
        self.dropout2 = torch.nn.Dropout(DROPOUT)
        self.fc1 = torch.nn.Sequential(torch.nn.Linear(hidden_size * 2, 128), torch.nn.Dropout(DROPOUT))
        self.bn = torch.nn.BatchNorm1d(128)
        self.fc2 = torch.nn.Sequential(torch.nn.Linear(128, out_channels), torch.nn.Tanh()) if use_tanh else torch.nn.Linear(128, out_channels)

    def forward(self, mels):
        y, _ = self.gru1(mels.transpose(1, 2))
        y, _ = self.gru2(self.dropout1(y))
        y = self.fc1(self.dropout2(y)).transpose(1, 2)
        y = self.bn(y).transpose(1, 2)
        return self.fc2(y).transpose(1, 2)

    def forward_rows(self, mels, lengths, valid):
        """The ragged step's forward from stock parts: each GRU layer over the packed sequences, fc1 / batch norm / fc2 on the valid rows
        only -> (M, out) in (b, t) order.  lengths: CPU int64; valid: (B, T) bool on the device."""
        T = mels.shape[2]
        y = mels.transpose(1, 2)
        for gru, drop in ((self.gru1, self.dropout1), (self.gru2, self.dropout2)):
            y, _ = gru(pack_padded_sequence(y, lengths, batch_first=True, enforce_sorted=False))
            y, _ = pad_packed_sequence(y, batch_first=True, total_length=T)
            y = drop(y)
        return self.fc2(self.bn(self.fc1(y[valid])))


def make_step(model, x, t):
    opt = torch.optim.Adam(model.parameters(), lr=1e-4, fused=True)

    def step():
        opt.zero_grad(set_to_none=True)
        F.l1_loss(model(x), t).backward()
        opt.step()

    return step


def ragged_main(a):
    """--ragged: see the module docstring."""
    params, B, T = SHAPES["full"], 32, 500
    lengths = torch.from_numpy(np.random.default_rng(a.seed).integers(100, T + 1, size=B)).to(torch.int64)
    M = int(lengths.sum())
    tsd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth_bigru_state_dict(params, seed=5101).items()}
    valid_cpu = torch.arange(T)[None, :] < lengths[:, None]
    valid = valid_cpu.cuda()
    x = torch.from_numpy(uniform(1, f"x.{B}.{T}", (B, params["in_channels"], T), -1.0, 1.0)) * valid_cpu[:, None, :]
    t = torch.from_numpy(uniform(1, f"t.{B}.{T}", (B, params["out_channels"], T), -1.0, 1.0)) * valid_cpu[:, None, :]
    x, t = x.cuda().contiguous(), t.cuda().contiguous()
    t_rows = t.transpose(1, 2)[valid].contiguous()
    lens32 = lengths.to(torch.int32)

    def native_model():
        m = BiGRU(**params, dropout=DROPOUT)
        m.load_state_dict(tsd, strict=True)
        return m.cuda().train()

    def make(model, loss_fn):
        opt = torch.optim.Adam(model.parameters(), lr=1e-4, fused=True)

        def step():
            opt.zero_grad(set_to_none=True)
            loss_fn(model).backward()
            opt.step()

        return step

    nr, nd = native_model(), native_model()
    legs = {"native_ragged": make(nr, lambda m: masked_l1_loss(m.forward_padded(x, lens32), t, lens32)),
            "native_dense": make(nd, lambda m: F.l1_loss(m(x), t))}
    if not a.no_stock:
        stock = StockBiGRU(**params)
        stock.load_state_dict(tsd, strict=True)
        legs["stock_ragged"] = make(stock.cuda().train(), lambda m: F.l1_loss(m.forward_rows(x, lengths, valid), t_rows))
    for _ in range(3):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(2):
        for k, fn in legs.items():
            ms[k].append(window(fn, a.window, a.limit))
    res = {"case": "ragged", "shape": "full", "B": B, "T": T, "seed": a.seed, "valid_frames": M, "padded_share": round(1.0 - M / (B * T), 4)}
    for k, v in ms.items():
        res[k + "_step_ms"] = [round(u, 3) for u in v]
        res[k + "_spread"] = round(abs(v[0] - v[1]) / min(v), 4)
    res["dense_over_ragged"] = round(min(ms["native_dense"]) / max(ms["native_ragged"]), 3)
    if "stock_ragged" in ms:
        res["stock_over_native_ragged"] = round(min(ms["stock_ragged"]) / max(ms["native_ragged"]), 3)  # slowest native, fastest stock
    for tag, m in (("ragged", nr), ("dense", nd)):
        prof = kernel_profile(m, legs["native_" + tag])
        res[tag + "_kernels_ms"] = {k: round(v, 4) for k, (_, v) in sorted(prof.items())}
        res[tag + "_kernels_total_ms"] = round(sum(v for _, v in prof.values()), 3)
        res[tag + "_fwd_sweep_us_per_step"] = round(prof.get("bigru_rec_kernel", (0, 0.0))[1] * 1e3 / (2 * T), 3)
        res[tag + "_bwd_sweep_us_per_step"] = round(prof.get("bigru_rec_bwd_kernel", (0, 0.0))[1] * 1e3 / (2 * T), 3)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


def lowrate_main(a):
    """--interp-factor N: see the module docstring."""
    params, N = SHAPES["full"], a.interp_factor
    tsd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth_bigru_state_dict(params, seed=5101).items()}
    cases = [(32, 500 // N * N)] if a.ragged else [(B, T) for B in a.batches for T in a.frames]
    lines = []
    for B, T in cases:
        if T % N:
            raise SystemExit(f"--frames {T} is no multiple of --interp-factor {N}")
        Tl = T // N
        xl = torch.from_numpy(uniform(1, f"xl.{B}.{Tl}", (B, params["in_channels"], Tl), -1.0, 1.0)).cuda()
        t = torch.from_numpy(uniform(1, f"t.{B}.{T}", (B, params["out_channels"], T), -1.0, 1.0)).cuda()
        lens = hi = None
        if a.ragged:
            lens = torch.from_numpy(np.random.default_rng(a.seed).integers(Tl // 5, Tl + 1, size=B)).to(torch.int32)
            hi = N * lens
            valid = (torch.arange(T)[None, :] < hi[:, None]).cuda()
            t = (t * valid[:, None, :]).contiguous()

        def native_model():
            m = BiGRU(**params, dropout=DROPOUT)
            m.load_state_dict(tsd, strict=True)
            return m.cuda().train()

        def make(model, fwd):
            opt = torch.optim.Adam(model.parameters(), lr=1e-4, fused=True)

            def step():
                opt.zero_grad(set_to_none=True)
                y = fwd(model)
                (F.l1_loss(y, t) if lens is None else masked_l1_loss(y, t, hi)).backward()
                opt.step()

            return step

        def stretched():
            return F.interpolate(xl, size=T, mode="linear", align_corners=False)

        ml, mm = native_model(), native_model()
        legs = {"lowrate": make(ml, lambda m: m.forward_lowrate_train(xl, lens, interp_factor=N)),
                "materialised": make(mm, (lambda m: m(stretched())) if lens is None else (lambda m: m.forward_padded(stretched(), hi)))}
        for _ in range(3):
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(2):
            for k, fn in legs.items():
                ms[k].append(window(fn, a.window, a.limit))
        res = {"case": "lowrate_ragged" if a.ragged else "lowrate", "shape": "full", "B": B, "Tl": Tl, "T": T, "interp_factor": N}
        if a.ragged:
            res.update(seed=a.seed, valid_low_frames=int(lens.sum()), padded_share=round(1.0 - int(lens.sum()) / (B * Tl), 4))
        for k, v in ms.items():
            res[k + "_step_ms"] = [round(u, 3) for u in v]
            res[k + "_spread_ms"] = round(abs(v[0] - v[1]), 3)
        gap = sum(ms["materialised"]) / 2 - sum(ms["lowrate"]) / 2
        spreads = abs(ms["lowrate"][0] - ms["lowrate"][1]) + abs(ms["materialised"][0] - ms["materialised"][1])
        res["materialised_minus_lowrate_ms"] = round(gap, 3)
        res["added_spreads_ms"] = round(spreads, 3)
        res["verdict"] = "not separated" if abs(gap) <= spreads else ("lowrate faster" if gap > 0 else "materialised faster")
        for tag, m in (("lowrate", ml), ("materialised", mm)):
            prof = kernel_profile(m, legs[tag])
            res[tag + "_kernels_ms"] = {k: round(v, 4) for k, (_, v) in sorted(prof.items())}
            res[tag + "_kernels_total_ms"] = round(sum(v for _, v in prof.values()), 3)
        lib, h = ml._lib, ml._handle
        res["lowrate_tape_bytes"] = int(lib.hificar_bigru_tape_bytes_lowrate(h, B, Tl, N))
        res["lowrate_workspace_bytes"] = int(lib.hificar_bigru_train_workspace_bytes_lowrate(h, B, Tl, N))
        res["materialised_tape_bytes"] = int(lib.hificar_bigru_tape_bytes(h, B, T))
        res["materialised_workspace_bytes"] = int(lib.hificar_bigru_train_workspace_bytes(h, B, T))
        res["materialised_stretched_input_bytes"] = B * params["in_channels"] * T * 4
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del ml, mm, legs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def window(fn, seconds, limit):
    """Mean device milliseconds per call over a window of at least `seconds` (events around blocks of calls)."""
    total_ms, calls, n = 0.0, 0, 1
    while total_ms < seconds * 1e3:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms / n > limit * 1e3:
            raise SystemExit(f"a step took {ms / n:.0f} ms, over the limit of {limit} s")
        total_ms += ms
        calls += n
        n = min(n * 2, 16)
    return total_ms / calls


def kernel_profile(m, fn):
    lib, eng = m._lib, m.engine()
    _native.check(lib.hificar_profile_begin(eng), "hificar_profile_begin")
    fn()
    return {r["name"]: (r["launches"], r["total_ms"]) for r in _native.profile_rows(lib, eng, 64)[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--frames", type=int, nargs="+", default=[200, 500])
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--limit", type=float, default=5.0, help="seconds a single step may take")
    ap.add_argument("--no-stock", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ragged", action="store_true", help="the ragged batch's three legs instead of the dense grid")
    ap.add_argument("--seed", type=int, default=0, help="--ragged: seed of the lengths")
    ap.add_argument("--interp-factor", type=int, default=1, help="> 1: the low-rate step against the materialised step (with --ragged: on a ragged batch)")
    a = ap.parse_args()
    if a.interp_factor != 1:
        _native.check_interp_factor(a.interp_factor)
        return lowrate_main(a)
    if a.ragged:
        return ragged_main(a)
    lines = []
    for shape in a.shapes:
        params = SHAPES[shape]
        tsd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth_bigru_state_dict(params, seed=5101).items()}
        for B in a.batches:
            for T in a.frames:
                native = BiGRU(**params, dropout=DROPOUT)
                native.load_state_dict(tsd, strict=True)
                native = native.cuda().train()
                x = torch.from_numpy(uniform(1, f"x.{B}.{T}", (B, params["in_channels"], T), -1.0, 1.0)).cuda()
                t = torch.from_numpy(uniform(1, f"t.{B}.{T}", (B, params["out_channels"], T), -1.0, 1.0)).cuda()
                nstep = make_step(native, x, t)
                sstep = None
                if not a.no_stock:
                    stock = StockBiGRU(**params)
                    stock.load_state_dict(tsd, strict=True)
                    sstep = make_step(stock.cuda().train(), x, t)
                for _ in range(3):
                    nstep()
                    if sstep:
                        sstep()
                torch.cuda.synchronize()
                n1 = window(nstep, a.window, a.limit)
                s1 = window(sstep, a.window, a.limit) if sstep else None
                n2 = window(nstep, a.window, a.limit)
                s2 = window(sstep, a.window, a.limit) if sstep else None
                res = {"shape": shape, "B": B, "T": T, "native_step_ms": [round(n1, 3), round(n2, 3)],
                       "native_spread": round(abs(n1 - n2) / min(n1, n2), 4)}
                if sstep:
                    res["stock_step_ms"] = [round(s1, 3), round(s2, 3)]
                    res["stock_spread"] = round(abs(s1 - s2) / min(s1, s2), 4)
                    res["stock_over_native"] = round(min(s1, s2) / max(n1, n2), 3)  # the conservative ratio: slowest native, fastest stock
                prof = kernel_profile(native, nstep)
                res["kernels_ms"] = {k: round(ms, 4) for k, (_, ms) in sorted(prof.items())}
                res["kernels_total_ms"] = round(sum(ms for _, ms in prof.values()), 3)
                res["fwd_sweep_us_per_step"] = round(prof.get("bigru_rec_kernel", (0, 0.0))[1] * 1e3 / (2 * T), 3)
                res["bwd_sweep_us_per_step"] = round(prof.get("bigru_rec_bwd_kernel", (0, 0.0))[1] * 1e3 / (2 * T), 3)
                res["tape_bytes"] = int(native._lib.hificar_bigru_tape_bytes(native._handle, B, T))
                res["workspace_bytes"] = int(native._lib.hificar_bigru_train_workspace_bytes(native._handle, B, T))
                lines.append(json.dumps(res))
                print(lines[-1], flush=True)
                del native, nstep, sstep
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
