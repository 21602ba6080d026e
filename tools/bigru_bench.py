#!/usr/bin/env python3
"""The BiGRU inversion model (articulatory_amd.models.BiGRU, C ABI hificar_bigru_*) at the published shape (1024, 256, 18), T = 2000.
   python tools/bigru_bench.py [--batches 1 8 64] [--frames 2000] [--window 0.5] [--cpu] [--out profiles/bigru.txt]

Per batch size B, device time from events, every shape warmed up first, windows of at least --window seconds:
  native   BiGRU.forward (libhificar.so)
  stock    the same model from stock PyTorch-ROCm modules on the same GPU (torch.nn.GRU x 2, Linear, BatchNorm1d, Linear — the reference's
           forward, pytorch_models.py:45-72); this restatement lives here, not in the package
alternated native / stock / native / stock in the same process: the two native windows run on unchanged code, and their difference is the
spread a ratio has to exceed.  Then, with hificar_profile_begin / hificar_profile_end on one native forward: time per kernel, the recurrent
kernel's time / (2 layers * T) = microseconds per step, and the projection GEMMs' share of the total.
--cpu adds the CPU restatement (the same torch modules on the host) at B = 1 with 1 and 16 threads.
--interp-factor N (with --frames as the LOW-RATE frame count, e.g. --frames 500 --interp-factor 4): the low-rate front end instead.  Two legs in
alternated windows a / b / a / b of one process, by device events:
  materialised  stock F.interpolate(size=N frames, mode='linear', align_corners=False) on the device, then BiGRU.forward: what a user does
                without the front end
  lowrate       BiGRU.forward_lowrate(x, interp_factor=N): layer 1's projection at the low rate, its pre-gates interpolated
Per leg: ms per forward, the per-kernel times of one forward from the library's event profile with the GEMMs' sum (the legs differ in layer
1's projection only), and the bytes of workspace (the materialised leg's stretched input counted with it).
HIFICAR_BIGRU_NS=1|2 overrides the number of sequences a workgroup sweeps (A/B runs of the tile height).
For per-kernel figures from the profiler instead:  rocprofv3 --kernel-trace --stats -- python tools/bigru_bench.py --batches 1 --window 0.05
Prints one JSON line per B; --out also appends them to a file."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from articulatory_amd import _native  # noqa: E402
from articulatory_amd.models import BiGRU  # noqa: E402
from articulatory_amd.utils.synth import synth_bigru_state_dict, uniform  # noqa: E402

PARAMS = dict(in_channels=1024, hidden_size=256, out_channels=18, use_tanh=False)


class StockBiGRU(torch.nn.Module):
    """The reference's module graph in eval mode (pytorch_models.py:27-37, 62-72) from stock torch.nn modules."""

    def __init__(self, in_channels, hidden_size, out_channels, use_tanh):
        super().__init__()
        self.gru1 = torch.nn.GRU(input_size=in_channels, hidden_size=hidden_size, num_layers=1, batch_first=True, bidirectional=True)
        self.gru2 = torch.nn.GRU(input_size=hidden_size * 2, hidden_size=hidden_size, num_layers=1, batch_first=True, bidirectional=True)
        self.fc1 = torch.nn.Sequential(torch.nn.Linear(hidden_size * 2, 128))
        self.bn = torch.nn.BatchNorm1d(128)
        self.fc2 = torch.nn.Sequential(torch.nn.Linear(128, out_channels), torch.nn.Tanh()) if use_tanh else torch.nn.Linear(128, out_channels)

    def forward(self, mels):
        y, _ = self.gru1(mels.transpose(1, 2))
        y, _ = self.gru2(y)
        y = self.fc1(y).transpose(1, 2)
        y = self.bn(y).transpose(1, 2)
        return self.fc2(y).transpose(1, 2)


def window(fn, x, seconds):
    """Mean device milliseconds per call over a window of at least `seconds` (events around blocks of calls)."""
    total_ms, calls, n = 0.0, 0, 1
    while total_ms < seconds * 1e3:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn(x)
        e1.record()
        e1.synchronize()
        total_ms += e0.elapsed_time(e1)
        calls += n
        n = min(n * 2, 64)
    return total_ms / calls


def kernel_profile(m, x, fn=None):
    lib, eng = m._lib, m.engine()
    _native.check(lib.hificar_profile_begin(eng), "hificar_profile_begin")
    (fn or m)(x)
    return {r["name"]: (r["launches"], r["total_ms"]) for r in _native.profile_rows(lib, eng, 32)[0]}


def lowrate_legs(native, B, Tl, f, seconds):
    """One JSON-able record of the two legs at batch size B (see the module docstring)."""
    import torch.nn.functional as F

    C = PARAMS["in_channels"]
    x = torch.from_numpy(uniform(1, f"bench.low.{B}", (B, C, Tl), -1.0, 1.0)).cuda()

    def materialised(x):
        return native(F.interpolate(x, size=f * Tl, mode="linear", align_corners=False))

    def lowrate(x):
        return native.forward_lowrate(x, interp_factor=f)

    ya, yb = materialised(x), lowrate(x)
    res = {"B": B, "Tl": Tl, "interp_factor": f, "T": f * Tl, "lowrate_vs_materialised_max_rel": float((ya - yb).abs().max() / ya.abs().max())}
    for _ in range(2):
        materialised(x), lowrate(x)
    torch.cuda.synchronize()
    a1 = window(materialised, x, seconds)
    b1 = window(lowrate, x, seconds)
    a2 = window(materialised, x, seconds)
    b2 = window(lowrate, x, seconds)
    res["materialised_ms"] = [round(a1, 4), round(a2, 4)]
    res["lowrate_ms"] = [round(b1, 4), round(b2, 4)]
    spread = abs(a1 - a2) + abs(b1 - b2)  # the two legs' window spreads, added: what a difference has to exceed
    diff = (b1 + b2) / 2 - (a1 + a2) / 2
    res["added_spread_ms"] = round(spread, 4)
    res["lowrate_minus_materialised_ms"] = round(diff, 4)
    res["verdict"] = "not separated" if abs(diff) <= spread else ("lowrate faster" if diff < 0 else "lowrate slower")
    res["materialised_over_lowrate"] = round(((a1 + a2) / 2) / ((b1 + b2) / 2), 3)
    lib, h = native._lib, native._native_handle()
    res["workspace_bytes"] = {"materialised": int(lib.hificar_bigru_workspace_bytes(h, B, f * Tl)) + 4 * B * C * f * Tl,
                              "lowrate": int(lib.hificar_bigru_workspace_bytes_lowrate(h, B, Tl, f))}
    for leg, fn in (("materialised", materialised), ("lowrate", lowrate)):
        prof = kernel_profile(native, x, fn)
        res[leg + "_kernels_ms"] = {k: round(ms, 4) for k, (_, ms) in sorted(prof.items())}
        res[leg + "_gemm_ms"] = round(sum(ms for k, (_, ms) in prof.items() if k.startswith("conv_")), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--no-stock", action="store_true")
    ap.add_argument("--interp-factor", type=int, default=None,
                    help="measure the low-rate front end: --frames low-rate frames stretched by this factor, materialised against forward_lowrate")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T = a.frames
    sd = synth_bigru_state_dict(PARAMS, seed=5101)
    tsd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    native = BiGRU(**PARAMS)
    native.load_state_dict(tsd, strict=True)
    native = native.eval().cuda()
    stock = StockBiGRU(**PARAMS)
    stock.load_state_dict(tsd, strict=True)
    stock_cpu = stock.eval()
    lines = []
    if a.interp_factor is not None:
        with torch.no_grad():
            for B in a.batches:
                lines.append(json.dumps(lowrate_legs(native, B, T, a.interp_factor, a.window)))
                print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    with torch.no_grad():
        if not a.no_stock:
            import copy
            stock = copy.deepcopy(stock_cpu).cuda()
        for B in a.batches:
            x = torch.from_numpy(uniform(1, f"bench.{B}", (B, PARAMS["in_channels"], T), -1.0, 1.0)).cuda()
            res = {"B": B, "T": T, "tile_height_env": os.environ.get("HIFICAR_BIGRU_NS")}
            y = native(x)
            if not a.no_stock:
                ys = stock(x)
                res["native_vs_stock_max_rel"] = float((y - ys).abs().max() / ys.abs().max())
                for _ in range(2):
                    native(x), stock(x)
            torch.cuda.synchronize()
            n1 = window(native, x, a.window)
            s1 = None if a.no_stock else window(stock, x, a.window)
            n2 = window(native, x, a.window)
            s2 = None if a.no_stock else window(stock, x, a.window)
            res["native_ms"] = [round(n1, 4), round(n2, 4)]
            res["native_frames_per_s"] = round(B * T / (min(n1, n2) * 1e-3))
            res["native_spread"] = round(abs(n1 - n2) / min(n1, n2), 4)
            if s1 is not None:
                res["stock_ms"] = [round(s1, 4), round(s2, 4)]
                res["stock_spread"] = round(abs(s1 - s2) / min(s1, s2), 4)
                res["stock_over_native"] = round(min(s1, s2) / max(n1, n2), 3)  # the conservative ratio: slowest native, fastest stock
            prof = kernel_profile(native, x)
            total = sum(ms for _, ms in prof.values())
            rec = prof.get("bigru_rec_kernel", (0, 0.0))[1]
            gemm = sum(ms for k, (_, ms) in prof.items() if k.startswith("conv_"))
            res["kernels_ms"] = {k: round(ms, 4) for k, (_, ms) in sorted(prof.items())}
            res["rec_us_per_step"] = round(rec * 1e3 / (2 * T), 3)
            res["gemm_share"] = round(gemm / total, 4) if total else None
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
        if a.cpu:
            x = torch.from_numpy(uniform(1, "bench.1", (1, PARAMS["in_channels"], T), -1.0, 1.0))
            for threads in (1, 16):
                torch.set_num_threads(threads)
                stock_cpu(x)
                t0 = time.perf_counter()
                reps = 0
                while time.perf_counter() - t0 < a.window or reps < 2:
                    stock_cpu(x)
                    reps += 1
                ms = (time.perf_counter() - t0) / reps * 1e3
                lines.append(json.dumps({"cpu_restatement_threads": threads, "B": 1, "T": T, "ms": round(ms, 2), "frames_per_s": round(T / (ms * 1e-3))}))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
