#!/usr/bin/env python3
"""What speaker conditioning costs in the AR loops: the width-512 e2w_hifigan_car generator with use_spk_id (32-dim embedding) against
the same model without, per AR step (chunk 25), through ``ar_synthesis`` and through ``StreamingSynthesizer.step()``, and the
conditioned batched loop against the Python loop of per-chunk batch-1 ``model(c, spk_id=, ar=prev)`` calls it replaces.

    python tools/cond_ar_bench.py [--frames 250] [--reps 7] [--batches 1 8 64]

Host clock around work that ends in a device synchronise; every shape is warmed up; the plain and the conditioned model alternate
inside each repetition; median and min..max over the repetitions are printed (the spread to read a difference against).  Needs a GPU."""

import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from articulatory_amd.models import HiFiGANGenerator  # noqa: E402
from articulatory_amd.streaming import StreamingSynthesizer  # noqa: E402
from articulatory_amd.utils.synth import synth_features, synth_state_dict  # noqa: E402

PARAMS = dict(in_channels=141, out_channels=1, channels=512, kernel_size=7, upsample_scales=[5, 4, 2, 2], upsample_kernel_sizes=[10, 8, 4, 4],
              resblock_kernel_sizes=[3, 7, 11], resblock_dilations=[[1, 3, 5]] * 3, use_additional_convs=True, bias=True,
              nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.1}, use_weight_norm=True, use_ar=True,
              ar_input=512, ar_hidden=256, ar_output=128)
CHUNK = 25
NUM_SPK = 8


def build(cond):
    p = dict(PARAMS, use_spk_id=True, num_spk=NUM_SPK, spk_emb_size=32) if cond else dict(PARAMS)
    g = HiFiGANGenerator(**p)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(p, seed=1234).items()})
    g.remove_weight_norm()
    return g.eval().to("cuda:0")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(ms):
    return f"{statistics.median(ms):8.3f} ms/step  ({min(ms):.3f} .. {max(ms):.3f})"


def stream_steps(g, cond, feats, spk, steps):
    """Sessions with all their frames buffered; returns the closure that runs the steps (the pushes are not timed)."""
    B = feats.shape[0]
    st = StreamingSynthesizer(g, CHUNK, max_sessions=B, ring_chunks=steps, conditioned=cond)
    for b in range(B):
        sid = st.open(**({"spk_id": int(spk[b])} if cond else {}))
        st.push(sid, feats[b])

    def run():
        for _ in range(steps):
            st.step()
    return run


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--loop-utterances", type=int, default=4, help="utterances of the Python per-chunk loop (batch 1 each)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cond_ar_bench: no GPU visible: nothing is measured on a CPU")
    steps = args.frames // CHUNK
    assert steps * CHUNK == args.frames, "--frames must be a multiple of 25"
    models = {False: build(False), True: build(True)}
    hop = models[True].hop
    print(f"# width-512 e2w_hifigan_car, fp32, chunk {CHUNK}, {args.frames} frames = {steps} steps per run, {args.reps} repetitions, "
          f"median (min .. max); plain and use_spk_id (32-dim, {NUM_SPK} speakers) alternate in every repetition")
    with torch.no_grad():
        for B in args.batches:
            feats = torch.from_numpy(synth_features(B, args.frames, 13, seed=B)).cuda()
            c = feats.permute(0, 2, 1).contiguous()
            spk = torch.arange(B, dtype=torch.int32, device="cuda:0") % NUM_SPK
            loop = {cond: (lambda cond=cond: models[cond].ar_synthesis(c, CHUNK, **({"spk_id": spk} if cond else {}))) for cond in models}
            res = {(kind, cond): [] for kind in ("ar_synthesis", "stream.step") for cond in models}
            for rep in range(args.reps + 1):  # repetition 0 warms every shape up
                for cond in models:
                    t = timed(loop[cond]) / steps
                    ts = timed(stream_steps(models[cond], cond, feats, spk.cpu(), steps)) / steps
                    if rep:
                        res[("ar_synthesis", cond)].append(t)
                        res[("stream.step", cond)].append(ts)
            for kind in ("ar_synthesis", "stream.step"):
                for cond in models:
                    print(f"batch {B:3d}  {kind:13s} {'use_spk_id' if cond else 'plain     '}  {summary(res[(kind, cond)])}")
                d = statistics.median(res[(kind, True)]) - statistics.median(res[(kind, False)])
                print(f"batch {B:3d}  {kind:13s} conditioned - plain = {d * 1e3:+.1f} us/step")
            if B == max(args.batches):
                sps = B * hop * CHUNK / (statistics.median(res[("ar_synthesis", True)]) * 1e-3)
                print(f"batch {B:3d}  conditioned batched loop: {sps / 1e6:.2f} M samples/s")
        # the loop this replaces: per-chunk forward calls, one utterance at a time
        g = models[True]
        U = args.loop_utterances
        feats = torch.from_numpy(synth_features(U, args.frames, 13, seed=99)).cuda()

        def python_loop():
            for u in range(U):
                prev = torch.zeros((1, 1, PARAMS["ar_input"]), device="cuda:0")
                sid = torch.tensor([u % NUM_SPK])
                outs = []
                for i in range(0, args.frames, CHUNK):
                    y = g(feats[u, i:i + CHUNK].t()[None].contiguous(), spk_id=sid, ar=prev)
                    outs.append(y[0, 0])
                    prev = y[:, :, -PARAMS["ar_input"]:]
                torch.cat(outs)

        ms = [timed(python_loop) for _ in range(args.reps + 1)][1:]
        sps = [U * hop * args.frames / (m * 1e-3) / 1e6 for m in ms]
        print(f"Python per-chunk loop, batch 1 ({U} utterances in turn): {statistics.median(sps):.2f} M samples/s  "
              f"({min(sps):.2f} .. {max(sps):.2f}); {statistics.median(ms) / (U * steps):.3f} ms/step")


if __name__ == "__main__":
    main()
