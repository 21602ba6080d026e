#!/usr/bin/env python3
"""The Transformer feature model (articulatory_amd.models.Transformer, C ABI hificar_xfmr_*) at the reference's default size (12 -> 80,
hidden 768, 6 layers), T = 2000.
   python tools/transformer_bench.py [--batches 1 8 32] [--frames 2000] [--window 0.5] [--out profiles/transformer.txt]

Per batch size B, device time from events, every shape warmed up first, windows of at least --window seconds:
  native   Transformer.forward (libhificar.so)
  stock    the same function from stock PyTorch-ROCm operators in fp32 on the same GPU: tests/transformer_oracle.py (conv1d, batch_norm,
           linear, einsum, softmax, layer_norm; the attention in its banded form, query chunks of 128 against the keys they can see)
alternated native / stock / native / stock in the same process: the two native windows run on unchanged code, and their difference is the
spread a ratio has to exceed.  The ratio reported is the conservative one: fastest stock window over slowest native window.  Then, with
hificar_profile_begin / hificar_profile_end on one native forward: time per kernel, the attention kernel's share of the forward and its
achieved TFLOP/s — counted as 2 * 3 * 199 * hidden FLOP per frame and layer (Q K^T, the positional product, P V over a full band) — against
the 157.3 TFLOP/s fp32 matrix peak.

   python tools/transformer_bench.py --precision bf16x3 [--out profiles/transformer_bf16x3.txt]

--precision bf16x3: a third leg, the same model with precision="bf16x3" (every GEMM in the conv engine's bf16x3 kernels), alternated
native-f32 / native-bf16x3 / stock, two windows each, in the same process.  Per B the line then also carries bf16x3_ms, the factor
f32_over_bf16x3 (fastest f32 window over slowest bf16x3 window: the conservative one), bf16x3_faster — the slowest bf16x3 window is
below the fastest f32 window by more than the two legs' window spreads added — the bf16x3 forward's error against the stock result,
and its own per-kernel table (bf16x3_kernels_ms) with the attention's and the GEMMs' shares.

   python tools/transformer_bench.py --precision bf16x3a [--out profiles/transformer_bf16x3a.txt]

--precision bf16x3a: the bf16x3 leg above AND one more, precision="bf16x3a" (the attention's products on bf16 MFMAs too, xfmr_attn16_kernel),
alternated native-f32 / native-bf16x3 / native-bf16x3a / stock, two windows each, in the same process: its yardstick is the bf16x3 leg of
the same run.  The line carries bf16x3a_ms, bf16x3_over_bf16x3a (fastest bf16x3 window over slowest bf16x3a window), bf16x3a_faster (the
slowest bf16x3a window is below the fastest bf16x3 window by more than the two legs' window spreads added), the error against the stock
result, the bf16x3a forward's per-kernel table, and per leg the profiled attention time and its share of the forward (attn_ms).

   python tools/transformer_bench.py --train [--shapes 8x200 32x500] [--out profiles/transformer_train.txt]

--train: one training step (forward in train() mode, dropout 0.2 + L1 loss + backward + fused Adam) at the same default size, per shape B x T,
native against stock alternated the same way.  Stock is tests/transformer_train_oracle.py in fp32 on the same GPU (conv1d, batch_norm,
linear, einsum, softmax, layer_norm under autograd, the attention banded too), its dropout masks drawn with torch.rand on the device (the
package's counter-based masks would be generated on the host).  The per-kernel profile covers one native forward + backward; the
attention backward's TFLOP/s counts 2 * 7 * 199 * hidden FLOP per frame and layer (S, dP, the K and E parts of dQ, dK, dV, dE).

   python tools/transformer_bench.py --train --ragged [--seed 0] [--full] [--out profiles/transformer_train_packed.txt]

--train --ragged: one batch of whole utterances instead — the default size, B 32, padded to T 500, lengths uniform in 100 .. 500 from --seed
(as tools/bigru_train_bench.py --ragged draws them; --full: every length = T) — and three legs of the same model in alternated windows: the
native packed step (Transformer.forward_padded(packed=True) + masked_l1_loss: no GEMM rows for the padding), the native ragged step
(forward_padded + masked_l1_loss) and the native dense step on the same padded batch (every frame counted, as the reference's pad mode
trains).  Then one profiled step of each: time per kernel, what the skipped attention tiles recover, the packed step's time over the
ragged step's per kernel family beside Mp / (B T), and the tape bytes of the three forms.

   python tools/transformer_bench.py --train --train-precision bf16x3 [--ragged] [--out profiles/transformer_train_bf16x3.txt]

--train-precision bf16x3 (with --train): one more leg, the same model with train_precision="bf16x3" (forward GEMMs and data gradients in the
bf16x3 kernels, fragments packed on the device after every optimizer step), alternated native-f32 / native-bf16x3 / stock, two windows
each, in the same process.  The line then carries bf16x3_ms, f32_over_bf16x3 (fastest f32 window over slowest bf16x3 window),
bf16x3_faster — the slowest bf16x3 window is below the fastest f32 window by more than the two legs' window spreads added — and the
bf16x3 step's per-kernel table (one forward + backward + the packs of one parameter hand-over).  With --ragged: the bf16x3 ragged and
packed legs beside the fp32 ones.

   python tools/transformer_bench.py --train --train-precision bf16x3w [--ragged] [--out profiles/transformer_train_bf16x3w.txt]

--train-precision bf16x3w: the bf16x3 leg(s) above AND one more, train_precision="bf16x3w" (the one-tap weight gradients on bf16 MFMAs too),
all in the same alternation: its yardsticks are the f32 and bf16x3 legs of the same run.  The line carries bf16x3w_ms,
bf16x3_over_bf16x3w (fastest bf16x3 window over slowest bf16x3w window), bf16x3w_faster (the slowest bf16x3w window is below the fastest
bf16x3 window by more than the two spreads added), the bf16x3w step's per-kernel table and wgrad_bf16x3_mfma_share: the bf16 MFMA issue
time of the new kernel's launches at the peak rate over their measured time.

   python tools/transformer_bench.py --train --train-precision bf16x3wa [--ragged] [--out profiles/transformer_train_bf16x3wa.txt]

--train-precision bf16x3wa: the bf16x3 and bf16x3w leg(s) above AND one more, train_precision="bf16x3wa" (the training attention's
query-tiled kernels on bf16 MFMAs too), in the same alternation: its yardstick is the bf16x3w leg of the same run.  The line carries
bf16x3wa_ms, bf16x3w_over_bf16x3wa (fastest bf16x3w window over slowest bf16x3wa window), bf16x3wa_faster (the slowest bf16x3wa window is
below the fastest bf16x3w window by more than the two spreads added), the bf16x3wa step's per-kernel table and attention_ms: the forward
(xfmr_attn16_kernel<train> against xfmr_attn_kernel<train>), the backward (xfmr_attn16_bwd_q_kernel + xfmr_attn_bwd_k_kernels against
xfmr_attn_bwd_kernels) and the tables' split (xfmr_split_tab_kernel, a cost) of the two legs' profiled steps.

   python tools/transformer_bench.py --train --train-precision bf16x3wac [--ragged] [--out profiles/transformer_train_bf16x3wac.txt]

--train-precision bf16x3wac: the bf16x3, bf16x3w and bf16x3wa leg(s) above AND one more, train_precision="bf16x3wac" (the wide k = 3 convs'
weight gradients on bf16 MFMAs too), in the same alternation: its yardstick is the bf16x3wa leg of the same run.  The line carries
bf16x3wac_ms, bf16x3wa_over_bf16x3wac (fastest bf16x3wa window over slowest bf16x3wac window), bf16x3wac_faster (the slowest bf16x3wac window
is below the fastest bf16x3wa window by more than the two spreads added), the bf16x3wac step's per-kernel table and conv_wgrad_ms: the moved
convs' rows of one bf16x3wa step (wgrad_taps_kernel and its reductions, by layer shape) beside those of one bf16x3wac step (the k3 rows of
wgrad_bf16x3_kernel, their reductions, xfmr_split_taps_t_kernel and what xfmr_split_rows_t_kernel takes above the bf16x3wa step's: the
moved layers' G splits), from two further models built under HIFICAR_PROFILE_DETAIL=1, which take no part in the timed windows.

   python tools/transformer_bench.py --train --train-precision bf16x3wack [--ragged] [--out profiles/transformer_train_bf16x3wack.txt]

--train-precision bf16x3wack: the bf16x3, bf16x3w, bf16x3wa and bf16x3wac leg(s) above AND one more, train_precision="bf16x3wack" (the
attention's key-tiled backward on bf16 MFMAs too), in the same alternation: its yardstick is the bf16x3wac leg of the same run.  The line
carries bf16x3wack_ms, bf16x3wac_over_bf16x3wack (fastest bf16x3wac window over slowest bf16x3wack window), bf16x3wack_faster (the slowest
bf16x3wack window is below the fastest bf16x3wac window by more than the two spreads added), the bf16x3wack step's per-kernel table and
key_tiled_ms: xfmr_attn_bwd_k_kernels of the bf16x3wac leg's profiled step beside xfmr_attn16_bwd_k_kernel and xfmr_demb16_partial_kernel of
the bf16x3wack leg's, and the ratio of the old row to the new pair's sum (below 1: the new pair is slower).
Reads nothing outside the repository.  Prints one JSON line per B; --out also appends them to a file."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from articulatory_amd import _native  # noqa: E402
from articulatory_amd.models import Transformer  # noqa: E402
from articulatory_amd.utils.synth import synth_transformer_state_dict, uniform  # noqa: E402
from transformer_oracle import TransformerOracle  # noqa: E402

PARAMS = dict(in_channels=12, out_channels=80, elayers=6, hidden_dim=768)
PEAK_TFLOPS = 157.3
BF16_PEAK_TFLOPS = 16 * PEAK_TFLOPS  # v_mfma_f32_32x32x16_bf16: 8 x the flops of 32x32x2_f32 in half its passes; wgrad_bf16x3_mfma_share divides by it


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


def kernel_profile(m, x):
    lib, eng = m._lib, m.engine()
    _native.check(lib.hificar_profile_begin(eng), "hificar_profile_begin")
    m(x)
    return {r["name"]: (r["launches"], r["total_ms"]) for r in _native.profile_rows(lib, eng, 128)[0]}


def attention_rows(pw, pa):
    """The attention's rows of a bf16x3w step's profile (pw) beside a bf16x3wa step's (pa): forward, backward, and the tables' split as a cost."""
    g = lambda prof, k: round(prof.get(k, 0.0), 4)  # noqa: E731
    return {"forward": {"bf16x3w xfmr_attn_kernel<train>": g(pw, "xfmr_attn_kernel<train>"), "bf16x3wa xfmr_attn16_kernel<train>": g(pa, "xfmr_attn16_kernel<train>")},
            "backward": {"bf16x3w xfmr_attn_bwd_kernels": g(pw, "xfmr_attn_bwd_kernels"), "bf16x3wa xfmr_attn16_bwd_q_kernel": g(pa, "xfmr_attn16_bwd_q_kernel"),
                         "bf16x3wa xfmr_attn_bwd_k_kernels": g(pa, "xfmr_attn_bwd_k_kernels")},
            "cost": {"bf16x3wa xfmr_split_tab_kernel": g(pa, "xfmr_split_tab_kernel")}}


def key_tiled_rows(pc, pk):
    """The key-tiled attention backward's rows of a bf16x3wac step's profile (pc) beside a bf16x3wack step's (pk)."""
    old = pc.get("xfmr_attn_bwd_k_kernels", 0.0)
    new = {k: round(pk.get(k, 0.0), 4) for k in ("xfmr_attn16_bwd_k_kernel", "xfmr_demb16_partial_kernel")}
    total = sum(new.values())
    return {"bf16x3wac xfmr_attn_bwd_k_kernels": round(old, 4), **{"bf16x3wack " + k: v for k, v in new.items()}, "bf16x3wack_sum": round(total, 4),
            "old_over_new": round(old / total, 3) if total else None}


def detail_profile(arith, sd, p, run):
    """{row: ms} of one step of a further model in `arith`, built under HIFICAR_PROFILE_DETAIL=1 (weight-gradient and reduction rows carry the
    layer's shape); run(m): one forward and backward.  The parameter hand-over behind an optimizer step lies inside the profile."""
    before = os.environ.get("HIFICAR_PROFILE_DETAIL")
    os.environ["HIFICAR_PROFILE_DETAIL"] = "1"
    try:
        m = Transformer(dropout=p, train_precision=arith, **PARAMS)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        m = m.cuda().train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-4, fused=True)
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            run(m)
            opt.step()
    finally:
        if before is None:
            del os.environ["HIFICAR_PROFILE_DETAIL"]
        else:
            os.environ["HIFICAR_PROFILE_DETAIL"] = before
    eng = m.engine()
    _native.check(m._lib.hificar_profile_begin(eng), "hificar_profile_begin")
    opt.zero_grad(set_to_none=True)
    run(m)
    return {r["name"]: r["total_ms"] for r in _native.profile_rows(m._lib, eng, 512)[0]}


def conv_wgrad_rows(pa, pc):
    """The moved k = 3 convs' rows of a bf16x3wa step's detailed profile (pa) beside a bf16x3wac step's (pc), and both sums."""
    shape = lambda r: r.split(" ")[1].split("p")[0]  # noqa: E731  ('kernel CxIkK[pP] ...')
    moved = {shape(r) for r in pc if r.startswith("wgrad_bf16x3_kernel") and "k3" in shape(r)}
    rows = lambda prof, pre: {r: round(v, 4) for r, v in sorted(prof.items()) if r.startswith(pre) and shape(r) in moved}  # noqa: E731
    old = rows(pa, ("wgrad_taps_kernel", "wreduce_"))
    new = rows(pc, ("wgrad_bf16x3_kernel", "wreduce_"))
    new["xfmr_split_taps_t_kernel"] = round(pc.get("xfmr_split_taps_t_kernel", 0.0), 4)
    new["xfmr_split_rows_t_kernel over bf16x3wa's"] = round(pc.get("xfmr_split_rows_t_kernel", 0.0) - pa.get("xfmr_split_rows_t_kernel", 0.0), 4)
    return {"bf16x3wa": old, "bf16x3wac": new, "bf16x3wa_sum": round(sum(old.values()), 4), "bf16x3wac_sum": round(sum(new.values()), 4)}


def train_main(a):
    import torch.nn.functional as F

    from transformer_train_oracle import TransformerTrainOracle

    class Stock(TransformerTrainOracle):
        def _mask(self, site, shape):
            if site % 4 == 0:
                shape = (shape[0], 8, shape[1], shape[1])
            return (torch.rand(shape, device=self.device) >= self.p).to(self.dtype) / (1.0 - self.p)

        def _relu(self, x, name):  # (without the restatement's bookkeeping, which synchronises)
            return torch.relu(x)

        def _bn(self, x, base, stats):
            q = self.params
            return F.batch_norm(x, self.buffers[base + ".running_mean"], self.buffers[base + ".running_var"], q[base + ".weight"], q[base + ".bias"],
                                training=True, momentum=0.1, eps=1e-5)

    p = 0.2
    sd = synth_transformer_state_dict(PARAMS, seed=6101)
    native = Transformer(dropout=p, **PARAMS)
    native.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    native = native.cuda().train()
    n_opt = torch.optim.Adam(native.parameters(), lr=1e-4, fused=True)
    stock = Stock(sd, dtype=torch.float32, device="cuda", dropout=p)
    s_opt = torch.optim.Adam(list(stock.params.values()), lr=1e-4, fused=True)
    fast = f_opt = None
    fastw = w_opt = None
    fastwa = wa_opt = None
    fastwac = wac_opt = None
    fastwack = wack_opt = None

    def leg(arith):
        m = Transformer(dropout=p, train_precision=arith, **PARAMS)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        m = m.cuda().train()
        return m, torch.optim.Adam(m.parameters(), lr=1e-4, fused=True)

    if a.train_precision in ("bf16x3", "bf16x3w", "bf16x3wa", "bf16x3wac", "bf16x3wack"):
        fast, f_opt = leg("bf16x3")
    if a.train_precision in ("bf16x3w", "bf16x3wa", "bf16x3wac", "bf16x3wack"):
        fastw, w_opt = leg("bf16x3w")
    if a.train_precision in ("bf16x3wa", "bf16x3wac", "bf16x3wack"):
        fastwa, wa_opt = leg("bf16x3wa")
    if a.train_precision in ("bf16x3wac", "bf16x3wack"):
        fastwac, wac_opt = leg("bf16x3wac")
    if a.train_precision == "bf16x3wack":
        fastwack, wack_opt = leg("bf16x3wack")

    def profile_step(m, opt):
        """{kernel: ms} of one step: the parameter hand-over behind the optimizer step before it, forward and backward."""
        eng = m.engine()
        opt.step()
        _native.check(m._lib.hificar_profile_begin(eng), "hificar_profile_begin")
        m.zero_grad(set_to_none=True)
        F.l1_loss(m(x), y).backward()
        rows, _ = _native.profile_rows(m._lib, eng, 128)
        profile_step.flops = {r["name"]: r["flops"] for r in rows}
        return {r["name"]: r["total_ms"] for r in rows}

    lines = []
    for shape in a.shapes:
        B, T = (int(v) for v in shape.split("x"))
        x = torch.from_numpy(uniform(1, f"bench.{B}", (B, PARAMS["in_channels"], T), -1.0, 1.0)).cuda()
        y = torch.from_numpy(uniform(2, f"bench.{B}", (B, PARAMS["out_channels"], T), -1.0, 1.0)).cuda()

        def native_step(_):
            n_opt.zero_grad(set_to_none=True)
            F.l1_loss(native(x), y).backward()
            n_opt.step()

        def stock_step(_):
            s_opt.zero_grad(set_to_none=True)
            F.l1_loss(stock.forward(x)[0], y).backward()
            s_opt.step()

        def fast_step(_):
            f_opt.zero_grad(set_to_none=True)
            F.l1_loss(fast(x), y).backward()
            f_opt.step()

        def fastw_step(_):
            w_opt.zero_grad(set_to_none=True)
            F.l1_loss(fastw(x), y).backward()
            w_opt.step()

        def fastwa_step(_):
            wa_opt.zero_grad(set_to_none=True)
            F.l1_loss(fastwa(x), y).backward()
            wa_opt.step()

        def fastwac_step(_):
            wac_opt.zero_grad(set_to_none=True)
            F.l1_loss(fastwac(x), y).backward()
            wac_opt.step()

        def fastwack_step(_):
            wack_opt.zero_grad(set_to_none=True)
            F.l1_loss(fastwack(x), y).backward()
            wack_opt.step()

        for _ in range(2):
            native_step(None), stock_step(None)
            if fast is not None:
                fast_step(None)
            if fastw is not None:
                fastw_step(None)
            if fastwa is not None:
                fastwa_step(None)
            if fastwac is not None:
                fastwac_step(None)
            if fastwack is not None:
                fastwack_step(None)
        torch.cuda.synchronize()
        n1 = window(native_step, None, a.window)
        f1 = None if fast is None else window(fast_step, None, a.window)
        w1 = None if fastw is None else window(fastw_step, None, a.window)
        a1 = None if fastwa is None else window(fastwa_step, None, a.window)
        c1 = None if fastwac is None else window(fastwac_step, None, a.window)
        k1 = None if fastwack is None else window(fastwack_step, None, a.window)
        s1 = window(stock_step, None, a.window)
        n2 = window(native_step, None, a.window)
        f2 = None if fast is None else window(fast_step, None, a.window)
        w2 = None if fastw is None else window(fastw_step, None, a.window)
        a2 = None if fastwa is None else window(fastwa_step, None, a.window)
        c2 = None if fastwac is None else window(fastwac_step, None, a.window)
        k2 = None if fastwack is None else window(fastwack_step, None, a.window)
        s2 = window(stock_step, None, a.window)
        res = {"train": True, "B": B, "T": T, "dropout": p, "native_ms": [round(n1, 3), round(n2, 3)], "stock_ms": [round(s1, 3), round(s2, 3)],
               "native_spread": round(abs(n1 - n2) / min(n1, n2), 4), "stock_spread": round(abs(s1 - s2) / min(s1, s2), 4),
               "stock_over_native": round(min(s1, s2) / max(n1, n2), 3), "native_frames_per_s": round(B * T / (min(n1, n2) * 1e-3))}
        lib, eng = native._lib, native.engine()
        _native.check(lib.hificar_profile_begin(eng), "hificar_profile_begin")
        native.zero_grad(set_to_none=True)
        F.l1_loss(native(x), y).backward()
        prof = {r["name"]: r["total_ms"] for r in _native.profile_rows(lib, eng, 128)[0]}
        total = sum(prof.values())
        res["kernels_share"] = {k: round(ms / total, 4) for k, ms in sorted(prof.items(), key=lambda kv: -kv[1])}
        res["profiled_total_ms"] = round(total, 3)
        bwd = prof.get("xfmr_attn_bwd_kernels", 0.0)
        flop = 2.0 * 7 * 199 * PARAMS["hidden_dim"] * B * T * PARAMS["elayers"]
        res["attn_bwd_ms"] = round(bwd, 3)
        res["attn_bwd_tflops"] = round(flop / (bwd * 1e-3) / 1e12, 2) if bwd else None
        if fast is not None:
            res["bf16x3_ms"] = [round(f1, 3), round(f2, 3)]
            res["bf16x3_spread"] = round(abs(f1 - f2) / min(f1, f2), 4)
            res["f32_over_bf16x3"] = round(min(n1, n2) / max(f1, f2), 3)
            res["stock_over_bf16x3"] = round(min(s1, s2) / max(f1, f2), 3)
            res["bf16x3_faster"] = bool(min(n1, n2) - max(f1, f2) > abs(n1 - n2) + abs(f1 - f2))
            pf, pn = profile_step(fast, f_opt), profile_step(native, n_opt)
            res["bf16x3_kernels_ms"] = {k: round(v, 4) for k, v in sorted(pf.items(), key=lambda kv: -kv[1])}
            res["f32_kernels_ms"] = {k: round(v, 4) for k, v in sorted(pn.items(), key=lambda kv: -kv[1])}
            fam = lambda prof, pre: round(sum(v for k, v in prof.items() if k.startswith(pre)), 4)  # noqa: E731
            res["families_ms"] = {pre: {"f32": fam(pn, pre), "bf16x3": fam(pf, pre)} for pre in ("conv", "wgrad", "wreduce", "xfmr_attn", "xfmr_split_rows", "pack16", "xfmr_")}
        if fastw is not None:
            res["bf16x3w_ms"] = [round(w1, 3), round(w2, 3)]
            res["bf16x3w_spread"] = round(abs(w1 - w2) / min(w1, w2), 4)
            res["f32_over_bf16x3w"] = round(min(n1, n2) / max(w1, w2), 3)
            res["bf16x3_over_bf16x3w"] = round(min(f1, f2) / max(w1, w2), 3)
            res["bf16x3w_faster"] = bool(min(f1, f2) - max(w1, w2) > abs(f1 - f2) + abs(w1 - w2))
            pw = profile_step(fastw, w_opt)
            res["bf16x3w_kernels_ms"] = {k: round(v, 4) for k, v in sorted(pw.items(), key=lambda kv: -kv[1])}
            for pre in res["families_ms"]:
                res["families_ms"][pre]["bf16x3w"] = fam(pw, pre)
            res["families_ms"]["xfmr_split_rows_t"] = {"f32": 0.0, "bf16x3": 0.0, "bf16x3w": fam(pw, "xfmr_split_rows_t")}
            # three bf16 MFMAs per fp32 product: the new kernel's bf16 MFMA issue time at the peak rate over its measured time
            wflops = sum(v for k, v in profile_step.flops.items() if k.startswith("wgrad_bf16x3"))
            wms = fam(pw, "wgrad_bf16x3")
            res["wgrad_bf16x3_mfma_share"] = round(3.0 * wflops / (BF16_PEAK_TFLOPS * 1e12) / (wms * 1e-3), 4) if wms else None
        if fastwa is not None:
            res["bf16x3wa_ms"] = [round(a1, 3), round(a2, 3)]
            res["bf16x3wa_spread"] = round(abs(a1 - a2) / min(a1, a2), 4)
            res["bf16x3w_over_bf16x3wa"] = round(min(w1, w2) / max(a1, a2), 3)
            res["bf16x3wa_faster"] = bool(min(w1, w2) - max(a1, a2) > abs(w1 - w2) + abs(a1 - a2))
            pa = profile_step(fastwa, wa_opt)
            res["bf16x3wa_kernels_ms"] = {k: round(v, 4) for k, v in sorted(pa.items(), key=lambda kv: -kv[1])}
            for pre in ("conv", "wgrad", "wreduce", "xfmr_attn", "xfmr_split_rows", "pack16", "xfmr_", "xfmr_split_rows_t"):
                res["families_ms"][pre]["bf16x3wa"] = fam(pa, pre)
            res["attention_ms"] = attention_rows(pw, pa)
        if fastwac is not None:
            res["bf16x3wac_ms"] = [round(c1, 3), round(c2, 3)]
            res["bf16x3wac_spread"] = round(abs(c1 - c2) / min(c1, c2), 4)
            res["bf16x3wa_over_bf16x3wac"] = round(min(a1, a2) / max(c1, c2), 3)
            res["bf16x3wac_faster"] = bool(min(a1, a2) - max(c1, c2) > abs(a1 - a2) + abs(c1 - c2))
            pc = profile_step(fastwac, wac_opt)
            res["bf16x3wac_kernels_ms"] = {k: round(v, 4) for k, v in sorted(pc.items(), key=lambda kv: -kv[1])}
            for pre in ("conv", "wgrad", "wreduce", "xfmr_attn", "xfmr_split_rows", "pack16", "xfmr_", "xfmr_split_rows_t"):
                res["families_ms"][pre]["bf16x3wac"] = fam(pc, pre)
            res["families_ms"]["xfmr_split_taps_t"] = {"bf16x3wa": 0.0, "bf16x3wac": fam(pc, "xfmr_split_taps_t")}
            run = lambda m: F.l1_loss(m(x), y).backward()  # noqa: E731
            res["conv_wgrad_ms"] = conv_wgrad_rows(detail_profile("bf16x3wa", sd, p, run), detail_profile("bf16x3wac", sd, p, run))
        if fastwack is not None:
            res["bf16x3wack_ms"] = [round(k1, 3), round(k2, 3)]
            res["bf16x3wack_spread"] = round(abs(k1 - k2) / min(k1, k2), 4)
            res["bf16x3wac_over_bf16x3wack"] = round(min(c1, c2) / max(k1, k2), 3)
            res["bf16x3wack_faster"] = bool(min(c1, c2) - max(k1, k2) > abs(c1 - c2) + abs(k1 - k2))
            pk = profile_step(fastwack, wack_opt)
            res["bf16x3wack_kernels_ms"] = {k: round(v, 4) for k, v in sorted(pk.items(), key=lambda kv: -kv[1])}
            for pre in ("conv", "wgrad", "wreduce", "xfmr_attn", "xfmr_split_rows", "pack16", "xfmr_", "xfmr_split_rows_t", "xfmr_split_taps_t"):
                res["families_ms"][pre]["bf16x3wack"] = fam(pk, pre)
            res["key_tiled_ms"] = key_tiled_rows(pc, pk)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def ragged_train_main(a):
    """--train --ragged: see the module docstring."""
    import torch.nn.functional as F

    from articulatory_amd.losses import masked_l1_loss

    p, B, T = 0.2, 32, 500
    lengths = torch.from_numpy(np.random.default_rng(a.seed).integers(100, T + 1, size=B)).to(torch.int64)
    if a.full:
        lengths = torch.full((B,), T, dtype=torch.int64)
    M = int(lengths.sum())
    valid = torch.arange(T)[None, :] < lengths[:, None]
    sd = synth_transformer_state_dict(PARAMS, seed=6101)
    m = Transformer(dropout=p, **PARAMS)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.cuda().train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-4, fused=True)
    x = (torch.from_numpy(uniform(1, f"bench.{B}", (B, PARAMS["in_channels"], T), -1.0, 1.0)) * valid[:, None, :]).cuda().contiguous()
    y = (torch.from_numpy(uniform(2, f"bench.{B}", (B, PARAMS["out_channels"], T), -1.0, 1.0)) * valid[:, None, :]).cuda().contiguous()
    lens32 = lengths.to(torch.int32)

    def make(loss_fn):
        def step(_=None):
            opt.zero_grad(set_to_none=True)
            loss_fn().backward()
            opt.step()

        return step

    legs = {"native_packed": make(lambda: masked_l1_loss(m.forward_padded(x, lens32, packed=True), y, lens32)),
            "native_ragged": make(lambda: masked_l1_loss(m.forward_padded(x, lens32), y, lens32)), "native_dense": make(lambda: F.l1_loss(m(x), y))}
    ariths = {"bf16x3": ("bf16x3",), "bf16x3w": ("bf16x3", "bf16x3w"), "bf16x3wa": ("bf16x3", "bf16x3w", "bf16x3wa"),
              "bf16x3wac": ("bf16x3", "bf16x3w", "bf16x3wa", "bf16x3wac"),
              "bf16x3wack": ("bf16x3", "bf16x3w", "bf16x3wa", "bf16x3wac", "bf16x3wack")}.get(a.train_precision, ())
    fast = {}
    for arith in ariths:  # the same batch through further models in the bf16x3 (and bf16x3w) training arithmetic, padded and packed
        m3 = Transformer(dropout=p, train_precision=arith, **PARAMS)
        m3.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        m3 = m3.cuda().train()
        opt3 = torch.optim.Adam(m3.parameters(), lr=1e-4, fused=True)
        fast[arith] = m3

        def make3(loss_fn, opt3=opt3):
            def step(_=None):
                opt3.zero_grad(set_to_none=True)
                loss_fn().backward()
                opt3.step()

            return step

        legs[arith + "_packed"] = make3(lambda m3=m3: masked_l1_loss(m3.forward_padded(x, lens32, packed=True), y, lens32))
        legs[arith + "_ragged"] = make3(lambda m3=m3: masked_l1_loss(m3.forward_padded(x, lens32), y, lens32))
    for _ in range(2):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(2):
        for k, fn in legs.items():
            ms[k].append(window(fn, None, a.window))
    tiles = sum((T + 63) // 64 - (int(n) + 63) // 64 for n in lengths)
    lib = m._lib
    Mp = int(lib.hificar_xfmr_packed_rows(B, T, lens32.data_ptr()))
    res = {"train": True, "case": "ragged", "B": B, "T": T, "dropout": p, "seed": a.seed, "full": bool(a.full), "valid_frames": M,
           "padded_share": round(1.0 - M / (B * T), 4), "skipped_attention_tiles": tiles, "attention_tiles": B * ((T + 63) // 64), "packed_rows": Mp,
           "packed_rows_over_padded_rows": round(Mp / (B * T), 4),
           "tape_bytes": {"packed": int(lib.hificar_xfmr_tape_bytes_packed(m._handle, B, Mp)), "ragged": int(lib.hificar_xfmr_tape_bytes(m._handle, B, T)),
                          "dense": int(lib.hificar_xfmr_tape_bytes(m._handle, B, T))}}
    for k, v in ms.items():
        res[k + "_step_ms"] = [round(u, 3) for u in v]
        res[k + "_spread"] = round(abs(v[0] - v[1]) / min(v), 4)
    res["dense_over_ragged"] = round(min(ms["native_dense"]) / max(ms["native_ragged"]), 3)  # slowest ragged, fastest dense
    res["ragged_over_packed"] = round(min(ms["native_ragged"]) / max(ms["native_packed"]), 3)  # slowest packed, fastest ragged
    res["packed_windows_below_ragged"] = max(ms["native_packed"]) < min(ms["native_ragged"])
    for form in ("packed", "ragged"):
        if "bf16x3_" + form in ms:
            n_, f_ = ms["native_" + form], ms["bf16x3_" + form]
            res[f"f32_over_bf16x3_{form}"] = round(min(n_) / max(f_), 3)
            res[f"bf16x3_faster_{form}"] = bool(min(n_) - max(f_) > abs(n_[0] - n_[1]) + abs(f_[0] - f_[1]))
        if "bf16x3w_" + form in ms:
            f_, w_ = ms["bf16x3_" + form], ms["bf16x3w_" + form]
            res[f"bf16x3_over_bf16x3w_{form}"] = round(min(f_) / max(w_), 3)
            res[f"bf16x3w_faster_{form}"] = bool(min(f_) - max(w_) > abs(f_[0] - f_[1]) + abs(w_[0] - w_[1]))
        if "bf16x3wa_" + form in ms:
            w_, a_ = ms["bf16x3w_" + form], ms["bf16x3wa_" + form]
            res[f"bf16x3w_over_bf16x3wa_{form}"] = round(min(w_) / max(a_), 3)
            res[f"bf16x3wa_faster_{form}"] = bool(min(w_) - max(a_) > abs(w_[0] - w_[1]) + abs(a_[0] - a_[1]))
        if "bf16x3wac_" + form in ms:
            a_, c_ = ms["bf16x3wa_" + form], ms["bf16x3wac_" + form]
            res[f"bf16x3wa_over_bf16x3wac_{form}"] = round(min(a_) / max(c_), 3)
            res[f"bf16x3wac_faster_{form}"] = bool(min(a_) - max(c_) > abs(a_[0] - a_[1]) + abs(c_[0] - c_[1]))
        if "bf16x3wack_" + form in ms:
            c_, k_ = ms["bf16x3wac_" + form], ms["bf16x3wack_" + form]
            res[f"bf16x3wac_over_bf16x3wack_{form}"] = round(min(c_) / max(k_), 3)
            res[f"bf16x3wack_faster_{form}"] = bool(min(c_) - max(k_) > abs(c_[0] - c_[1]) + abs(k_[0] - k_[1]))
    eng = m.engine()
    profs = {}
    for tag in ("packed", "ragged", "dense"):
        _native.check(lib.hificar_profile_begin(eng), "hificar_profile_begin")
        legs["native_" + tag]()
        profs[tag] = {r["name"]: r["total_ms"] for r in _native.profile_rows(lib, eng, 128)[0]}
        res[tag + "_kernels_ms"] = {k: round(v, 4) for k, v in sorted(profs[tag].items(), key=lambda kv: -kv[1])}
        res[tag + "_kernels_total_ms"] = round(sum(profs[tag].values()), 3)
    for arith, m3 in fast.items():
        eng3 = m3.engine()
        for tag in ("packed", "ragged"):
            _native.check(lib.hificar_profile_begin(eng3), "hificar_profile_begin")
            legs[f"{arith}_{tag}"]()
            prof3 = {r["name"]: r["total_ms"] for r in _native.profile_rows(lib, eng3, 128)[0]}
            res[f"{arith}_{tag}_kernels_ms"] = {k: round(v, 4) for k, v in sorted(prof3.items(), key=lambda kv: -kv[1])}
            res[f"{arith}_{tag}_kernels_total_ms"] = round(sum(prof3.values()), 3)
    if "bf16x3wa" in fast:
        res["attention_ms"] = {tag: attention_rows(res[f"bf16x3w_{tag}_kernels_ms"], res[f"bf16x3wa_{tag}_kernels_ms"]) for tag in ("packed", "ragged")}
    if "bf16x3wac" in fast:
        runs = {"packed": lambda m3: masked_l1_loss(m3.forward_padded(x, lens32, packed=True), y, lens32).backward(),
                "ragged": lambda m3: masked_l1_loss(m3.forward_padded(x, lens32), y, lens32).backward()}
        res["conv_wgrad_ms"] = {tag: conv_wgrad_rows(detail_profile("bf16x3wa", sd, p, run), detail_profile("bf16x3wac", sd, p, run)) for tag, run in runs.items()}
    if "bf16x3wack" in fast:
        res["key_tiled_ms"] = {tag: key_tiled_rows(res[f"bf16x3wac_{tag}_kernels_ms"], res[f"bf16x3wack_{tag}_kernels_ms"]) for tag in ("packed", "ragged")}
    res["attention_recovered_ms"] = {k: round(profs["dense"].get(k, 0.0) - profs["ragged"].get(k, 0.0), 4)
                                     for k in ("xfmr_attn_kernel<train>", "xfmr_attn_bwd_kernels")}
    # packed over ragged per kernel family, to read beside packed_rows_over_padded_rows: conv_* are the forward GEMMs and the data gradients
    fam = lambda prof, pre: sum(v for k, v in prof.items() if k.startswith(pre))  # noqa: E731
    res["packed_over_ragged_ms"] = {k: round(profs["packed"].get(k, 0.0) / v, 4) for k, v in profs["ragged"].items() if v > 0}
    res["packed_over_ragged_families"] = {pre: round(fam(profs["packed"], pre) / fam(profs["ragged"], pre), 4) for pre in ("conv", "wgrad", "xfmr_attn", "xfmr_")
                                          if fam(profs["ragged"], pre) > 0}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--shapes", nargs="+", default=["8x200", "32x500"])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--no-stock", action="store_true")
    ap.add_argument("--precision", choices=("f32", "bf16x3", "bf16x3a"), default="f32",
                    help="bf16x3: add the bf16x3 leg to the native / stock alternation; bf16x3a: that leg and the bf16x3a leg")
    ap.add_argument("--train-precision", choices=("f32", "bf16x3", "bf16x3w", "bf16x3wa", "bf16x3wac", "bf16x3wack"), default="f32",
                    help="--train: bf16x3 adds the bf16x3 training leg(s); bf16x3w adds those and the bf16x3w leg(s); bf16x3wa those and the bf16x3wa leg(s); "
                         "bf16x3wac those and the bf16x3wac leg(s); bf16x3wack those and the bf16x3wack leg(s)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ragged", action="store_true", help="--train: the ragged batch's two legs instead of the dense shapes")
    ap.add_argument("--seed", type=int, default=0, help="--train --ragged: seed of the lengths")
    ap.add_argument("--full", action="store_true", help="--train --ragged: every length = T (what the gap and rounding rows cost)")
    a = ap.parse_args()
    if a.ragged and not a.train:
        ap.error("--ragged goes with --train")
    if a.train and a.ragged:
        return ragged_train_main(a)
    if a.train:
        return train_main(a)
    T = a.frames
    sd = synth_transformer_state_dict(PARAMS, seed=6101)
    native = Transformer(**PARAMS)
    native.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    native = native.eval().cuda()
    fast = None
    fasta = None
    if a.precision in ("bf16x3", "bf16x3a"):
        fast = Transformer(**PARAMS, precision="bf16x3")
        fast.load_state_dict(native.state_dict(), strict=True)
        fast = fast.eval().cuda()
    if a.precision == "bf16x3a":
        fasta = Transformer(**PARAMS, precision="bf16x3a")
        fasta.load_state_dict(native.state_dict(), strict=True)
        fasta = fasta.eval().cuda()
    stock = None if a.no_stock else TransformerOracle(sd, dtype=torch.float32, device="cuda").forward
    lines = []
    with torch.no_grad():
        for B in a.batches:
            x = torch.from_numpy(uniform(1, f"bench.{B}", (B, PARAMS["in_channels"], T), -1.0, 1.0)).cuda()
            res = {"B": B, "T": T}
            y = native(x)
            if stock is not None:
                ys = stock(x)
                res["native_vs_stock_max_rel"] = float((y - ys).abs().max() / ys.abs().max())
                for _ in range(2):
                    native(x), stock(x)
            if fast is not None:
                yf = fast(x)
                res["bf16x3_vs_f32_max_rel"] = float((yf - y).abs().max() / y.abs().max())
                if stock is not None:
                    res["bf16x3_vs_stock_max_rel"] = float((yf - ys).abs().max() / ys.abs().max())
                for _ in range(2):
                    fast(x)
            if fasta is not None:
                ya = fasta(x)
                res["bf16x3a_vs_f32_max_rel"] = float((ya - y).abs().max() / y.abs().max())
                res["bf16x3a_vs_bf16x3_max_rel"] = float((ya - yf).abs().max() / y.abs().max())
                if stock is not None:
                    res["bf16x3a_vs_stock_max_rel"] = float((ya - ys).abs().max() / ys.abs().max())
                for _ in range(2):
                    fasta(x)
            torch.cuda.synchronize()
            n1 = window(native, x, a.window)
            f1 = None if fast is None else window(fast, x, a.window)
            a1 = None if fasta is None else window(fasta, x, a.window)
            s1 = None if stock is None else window(stock, x, a.window)
            n2 = window(native, x, a.window)
            f2 = None if fast is None else window(fast, x, a.window)
            a2 = None if fasta is None else window(fasta, x, a.window)
            s2 = None if stock is None else window(stock, x, a.window)
            res["native_ms"] = [round(n1, 4), round(n2, 4)]
            res["native_frames_per_s"] = round(B * T / (min(n1, n2) * 1e-3))
            res["native_spread"] = round(abs(n1 - n2) / min(n1, n2), 4)
            if s1 is not None:
                res["stock_ms"] = [round(s1, 4), round(s2, 4)]
                res["stock_spread"] = round(abs(s1 - s2) / min(s1, s2), 4)
                res["stock_over_native"] = round(min(s1, s2) / max(n1, n2), 3)
            prof = kernel_profile(native, x)
            total = sum(ms for _, ms in prof.values())
            attn = prof.get("xfmr_attn_kernel", (0, 0.0))[1]
            gemm = sum(ms for k, (_, ms) in prof.items() if k.startswith("conv_"))
            res["kernels_ms"] = {k: round(ms, 4) for k, (_, ms) in sorted(prof.items())}
            res["profiled_total_ms"] = round(total, 4)
            res["attn_share"] = round(attn / total, 4) if total else None
            res["gemm_share"] = round(gemm / total, 4) if total else None
            flop = 2.0 * 3 * 199 * PARAMS["hidden_dim"] * B * T * PARAMS["elayers"]
            res["attn_tflops"] = round(flop / (attn * 1e-3) / 1e12, 2) if attn else None
            res["attn_of_peak"] = round(flop / (attn * 1e-3) / 1e12 / PEAK_TFLOPS, 4) if attn else None
            if fast is not None:
                res["bf16x3_ms"] = [round(f1, 4), round(f2, 4)]
                res["bf16x3_frames_per_s"] = round(B * T / (min(f1, f2) * 1e-3))
                res["bf16x3_spread"] = round(abs(f1 - f2) / min(f1, f2), 4)
                res["f32_over_bf16x3"] = round(min(n1, n2) / max(f1, f2), 3)
                res["bf16x3_faster"] = bool(min(n1, n2) - max(f1, f2) > abs(n1 - n2) + abs(f1 - f2))
                if s1 is not None:
                    res["stock_over_bf16x3"] = round(min(s1, s2) / max(f1, f2), 3)
                fprof = kernel_profile(fast, x)
                ftotal = sum(ms for _, ms in fprof.values())
                fattn = fprof.get("xfmr_attn_kernel<split>", (0, 0.0))[1]
                res["bf16x3_kernels_ms"] = {k: round(ms, 4) for k, (_, ms) in sorted(fprof.items())}
                res["bf16x3_profiled_total_ms"] = round(ftotal, 4)
                res["bf16x3_attn_share"] = round(fattn / ftotal, 4) if ftotal else None
                res["bf16x3_gemm_share"] = round(sum(ms for k, (_, ms) in fprof.items() if k.startswith("conv_")) / ftotal, 4) if ftotal else None
            if fasta is not None:
                res["bf16x3a_ms"] = [round(a1, 4), round(a2, 4)]
                res["bf16x3a_frames_per_s"] = round(B * T / (min(a1, a2) * 1e-3))
                res["bf16x3a_spread"] = round(abs(a1 - a2) / min(a1, a2), 4)
                res["bf16x3_over_bf16x3a"] = round(min(f1, f2) / max(a1, a2), 3)
                res["bf16x3a_faster"] = bool(min(f1, f2) - max(a1, a2) > abs(f1 - f2) + abs(a1 - a2))
                if s1 is not None:
                    res["stock_over_bf16x3a"] = round(min(s1, s2) / max(a1, a2), 3)
                aprof = kernel_profile(fasta, x)
                atotal = sum(ms for _, ms in aprof.values())
                aattn = aprof.get("xfmr_attn16_kernel", (0, 0.0))[1]
                res["bf16x3a_kernels_ms"] = {k: round(ms, 4) for k, (_, ms) in sorted(aprof.items())}
                res["bf16x3a_profiled_total_ms"] = round(atotal, 4)
                res["bf16x3a_attn_share"] = round(aattn / atotal, 4) if atotal else None
                res["bf16x3a_gemm_share"] = round(sum(ms for k, (_, ms) in aprof.items() if k.startswith("conv_")) / atotal, 4) if atotal else None
                # the attention kernel's own profiled time and its share of the forward, per leg
                res["attn_ms"] = {"f32": [round(attn, 4), res["attn_share"]], "bf16x3": [round(fattn, 4), res["bf16x3_attn_share"]],
                                  "bf16x3a": [round(aattn, 4), res["bf16x3a_attn_share"]]}
                res["attn_bf16x3_over_bf16x3a"] = round(fattn / aattn, 3) if aattn else None
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
