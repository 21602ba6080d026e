#!/usr/bin/env python3
"""Streaming synthesis (articulatory_amd.streaming, C ABI hificar_ar_step) at S live sessions vs the same batch through ar_synthesis.
   HIFICAR_AR_DUAL_MAX=0 python tools/stream_bench.py [--sessions 1 8 64] [--chunk 25] [--precision f32]

Per S, on the e2w recipe shape:
  live    S sessions with staggered starts (session i joins at round i * 8 // S) fed random packets of 1 .. 3*chunk frames per round,
          one step() per round: host time of step() (perf_counter) over the rounds in which all S sessions advanced.
  device  device time per step from events: blocks of 8 steps of all S sessions (frames pushed beforehand, a _sleep in front so that
          the host has queued the whole block), alternated in the same process with blocks of 8 one-chunk ar_synthesis calls of S
          utterances.  Run with HIFICAR_AR_DUAL_MAX=0 so that ar_synthesis runs on one stream, as a step does.
Prints one JSON line per S."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from articulatory_amd.models import HiFiGANGenerator  # noqa: E402
from articulatory_amd.streaming import StreamingSynthesizer  # noqa: E402
from articulatory_amd.utils.synth import synth_features, synth_state_dict  # noqa: E402
from bench import CAR_PARAMS  # noqa: E402

BLOCK = 8


def live(g, S, chunk, rounds, seed):
    st = StreamingSynthesizer(g, chunk, max_sessions=S, ring_chunks=4)
    rng = np.random.default_rng(seed)
    feats = torch.from_numpy(synth_features(1, 4 * chunk, 13, seed=seed)[0]).cuda()
    sids = []
    host = []
    for r in range(rounds):
        while len(sids) < S and len(sids) * 8 // S <= r:
            sids.append(st.open())
        for sid in sids:
            n = min(int(rng.integers(1, 3 * chunk + 1)), st.sched.ring_frames - st.sched.buffered(sid))
            if n > 0:
                st.push(sid, feats[:n])
        t0 = time.perf_counter()
        out = st.step()
        dt = time.perf_counter() - t0
        if len(out) == S and r >= 8:
            host.append(dt * 1e3)
    torch.cuda.synchronize()
    return host


def device_blocks(g, S, chunk, reps):
    st = StreamingSynthesizer(g, chunk, max_sessions=S, ring_chunks=BLOCK)
    sids = [st.open() for _ in range(S)]
    feats = torch.from_numpy(synth_features(1, BLOCK * chunk, 13, seed=5)[0]).cuda()
    c = torch.from_numpy(synth_features(S, chunk, 13, seed=6)).permute(0, 2, 1).contiguous().cuda()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * BLOCK)]
    stream_ms, offline_ms = [], []

    def block(fn):
        torch.cuda.synchronize()
        torch.cuda._sleep(20_000_000)
        for i in range(BLOCK):
            ev[2 * i].record()
            fn()
            ev[2 * i + 1].record()
        torch.cuda.synchronize()
        return [ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(BLOCK)]

    for sid in sids:  # warm-up: launch shapes' schedules, staging ring
        st.push(sid, feats[:chunk])
    st.step()
    g.ar_synthesis(c, chunk)
    for _ in range(reps):
        for sid in sids:
            st.push(sid, feats)

        def one_step():
            assert len(st.step()) == S

        stream_ms += block(one_step)
        offline_ms += block(lambda: g.ar_synthesis(c, chunk))
    return stream_ms, offline_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--chunk", type=int, default=25)
    ap.add_argument("--precision", default="f32")
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--reps", type=int, default=6)
    a = ap.parse_args()
    if os.environ.get("HIFICAR_AR_DUAL_MAX") != "0":
        print("note: HIFICAR_AR_DUAL_MAX is not 0: ar_synthesis may run a batch as two halves on two streams", file=sys.stderr)
    sd = synth_state_dict(CAR_PARAMS, seed=1234)
    g = HiFiGANGenerator(**CAR_PARAMS, precision=a.precision)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    g.remove_weight_norm()
    g = g.eval().cuda()
    with torch.no_grad():
        for S in a.sessions:
            host = live(g, S, a.chunk, a.rounds, seed=S)
            sm, om = device_blocks(g, S, a.chunk, a.reps)
            med_s, med_o = float(np.median(sm)), float(np.median(om))
            print(json.dumps(dict(sessions=S, chunk=a.chunk, precision=a.precision,
                                  step_device_ms=round(med_s, 4), ar_synthesis_step_device_ms=round(med_o, 4),
                                  device_ratio=round(med_s / med_o, 4),
                                  step_host_ms=round(float(np.median(host)), 4) if host else None, full_live_steps=len(host),
                                  device_ms_p10_p90=[round(float(np.percentile(sm, q)), 4) for q in (10, 90)],
                                  ar_synthesis_ms_p10_p90=[round(float(np.percentile(om, q)), 4) for q in (10, 90)])), flush=True)


if __name__ == "__main__":
    main()
