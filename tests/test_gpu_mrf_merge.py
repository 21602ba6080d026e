"""The branch-summing last ResBlock launch (conv_f32mrg_kernel, csrc/hificar_conv.hip.h) and the one-stream upsampler behind it.  ``pytest -m gpu``.

Exact fp32 inference may run the last conv2 launch of a stage with all residual blocks summed in one accumulator: the workgroup that owns an output
position runs the K loops of every block and stores LeakyReLU(mean) once, so the next upsampler stages one activated stream by LDS-DMA.  The planner
takes that form only for launches that fill the chip, so every model here is built with HIFICAR_MRF_MERGE=2 (the form wherever the rules allow it),
set — like HIFICAR_PROFILE_DETAIL=1, which makes the profile rows carry "kernel|layer +N" — before the model's native handle exists.

The merged form adds the blocks in another order than the layer-by-layer path (which rounds every block's output to fp32 first), so the two agree to
fp32 rounding: the tolerances are the project's own for the same comparison in test_gpu_parity.py::test_mrf_mean_folded_into_the_upsampler, 2e-5
against the oracle and 5e-6 between two forwards (both rel_err), and XSHAPE_TOL between launches of different shapes."""

import re

import numpy as np
import pytest
import torch

from conftest import E2W_PARAMS, rel_err, same_across_shapes
from articulatory_amd.models import HiFiGANGenerator
from articulatory_amd.streaming import StreamingSynthesizer
from articulatory_amd.utils.synth import synth_features, synth_state_dict
from oracle import hificar_oracle as O
from test_gpu_conv_tiles import GEN_B, GEN_HOP, GEN_LENS, GEN_PARAMS, GEN_SEED, GEN_T, SHAPES, Layer, _round_up, admissible, force, shape_id
from test_gpu_parity import XSHAPE_TOL

pytestmark = pytest.mark.gpu

ORACLE_TOL = 2e-5
FORWARD_TOL = 5e-6
MRG = "conv_f32mrg_kernel"


def build(env, params=GEN_PARAMS, remove_wn=True, seed=1234):
    """A model whose native handle is built under the switches `env` (on top of HIFICAR_PROFILE_DETAIL=1; every other switch unset)."""
    assert torch.cuda.is_available(), "these tests need a GPU; run with -m 'not gpu' on CPU boxes"
    mp = pytest.MonkeyPatch()
    try:
        for name in ("HIFICAR_MRF_MERGE", "HIFICAR_PAIR", "HIFICAR_KSPLIT", "HIFICAR_PAIR_SMALL", "HIFICAR_LAUNCH_LOG"):
            mp.delenv(name, raising=False)
        mp.setenv("HIFICAR_PROFILE_DETAIL", "1")
        for name, value in env.items():
            mp.setenv(name, value)
        sd = synth_state_dict(params, seed=seed)
        g = HiFiGANGenerator(**params, precision="f32")
        g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        if remove_wn:
            g.remove_weight_norm()
        g = g.eval().to("cuda:0")
        g._native_handle()  # (the switches are read here)
    finally:
        mp.undo()
    return g, sd


# stage widths 32 / 16 / 8 / 4, every one padded to a 32-channel row pitch: the merged launches of stages 0 - 2 run the 16-channel K chunk (NC16 = 1)
NARROW_PARAMS = dict(GEN_PARAMS, channels=64)


def kernels_params(kernels):
    return dict(GEN_PARAMS, resblock_kernel_sizes=kernels, resblock_dilations=[[1, 3, 5]] * len(kernels))


def gen_inputs(B=GEN_B, T=GEN_T, seed=GEN_SEED):
    c = torch.from_numpy(synth_features(B, T, 13, seed=seed)).permute(0, 2, 1).contiguous()
    ar = torch.from_numpy(synth_features(B, 512, 1, seed=seed + 1)[:, :, 0] * 0.3).reshape(B, 1, 512)
    return c, ar


def profiled(g, fn):
    """fn() under the profiler: (result, {"layer xN" / "layer +N": (kernel, launches, bytes)}, names of the other kernels).  For windows in which
    every layer is launched at one shape."""
    g.profile_begin()
    try:
        out = fn()
    finally:
        stats = g.profile_end()
    rows, others = {}, set()
    for s in stats:
        if "|" in s["name"]:
            kernel, layer = s["name"].split("|")
            assert layer not in rows, (layer, kernel)
            rows[layer] = (kernel, s["launches"], s["bytes"])
        else:
            others.add(s["name"])
    return out, rows, others


def merged_rows(rows):
    return {layer: v for layer, v in rows.items() if v[0].startswith(MRG)}


def expect_merged(params, stages):
    """The profile labels of the merged launches of `stages`: the stage's last conv2 layer of the heaviest (= first launched) block, "+n"."""
    ks = params["resblock_kernel_sizes"]
    n, last = len(ks), len(params["resblock_dilations"][0]) - 1
    heaviest = max(range(n), key=lambda j: (ks[j], -j))
    return ["blocks.%d.convs2.%d.1 +%d" % (i * n + heaviest, last, n) for i in stages]


def check_forms(params, rows_on, rows_off, stages, B, T):
    """Stages `stages` ran their last layer as ONE merged launch and nothing of it side by side; the upsampler behind each staged one input
    stream — the library's byte count of that launch is smaller than the layer-by-layer model's by exactly the n - 1 further streams."""
    n = len(params["resblock_kernel_sizes"])
    assert sorted(merged_rows(rows_on)) == sorted(expect_merged(params, stages)), sorted(rows_on)
    assert not merged_rows(rows_off)
    last = len(params["resblock_dilations"][0]) - 1
    rows_in = T if T <= 32 else _round_up(T, 32)  # (a launch covers a bucket of frames)
    for i, s in enumerate(params["upsample_scales"]):
        rows_in *= s  # rows of stage i = input rows of upsampler i + 1
        if i not in stages:
            continue
        for j in range(n):  # no block's last conv2 layer as a side-by-side row
            assert not any(layer.startswith("blocks.%d.convs2.%d.1 x" % (i * n + j, last)) for layer in rows_on), (i, j)
        up = "upsamples.%d.1 x1" % (i + 1)
        cin_pad = _round_up(params["channels"] >> (i + 1), 32)
        assert rows_on[up][1] == rows_off[up][1]
        assert rows_off[up][2] - rows_on[up][2] == 4.0 * B * rows_in * cin_pad * (n - 1) * rows_on[up][1], (up, rows_on[up], rows_off[up])


# ------------------------------------------------------------------------------------------------ 1. oracle and the layer-by-layer path
FORWARD_CASES = {"k3_7_11": kernels_params([3, 7, 11]), "k3_7": kernels_params([3, 7]), "k3_5_7_11": kernels_params([3, 5, 7, 11]), "narrow_chunk16": NARROW_PARAMS}


@pytest.mark.parametrize("case", sorted(FORWARD_CASES))
def test_merged_forward_against_oracle_and_classic(case):
    """2, 3 and 4 blocks per stage on the small model of test_gpu_conv_tiles.py (stage widths 192 / 96 / 48 / 24: K chunks 64 / 32 / 32 / 16, partial
    channel groups; 31 frames: a partial last row tile at every height), and its narrow sibling whose merged launches run 16-channel K chunks: the waveform against the oracle and against the same model built with
    HIFICAR_MRF_MERGE=0; every non-last stage's last layer ran merged, the upsamplers behind them on one stream."""
    params = FORWARD_CASES[case]
    g_on, sd = build({"HIFICAR_MRF_MERGE": "2"}, params)
    g_off, _ = build({"HIFICAR_MRF_MERGE": "0"}, params)
    c, ar = gen_inputs()
    with torch.no_grad():
        y_on, rows_on, _ = profiled(g_on, lambda: g_on(c.cuda(), ar=ar.cuda()))
        y_off, rows_off, _ = profiled(g_off, lambda: g_off(c.cuda(), ar=ar.cuda()))
        ref = O.generator_forward(O.fold_weight_norm(sd), params, c, ar)
    check_forms(params, rows_on, rows_off, [0, 1, 2], GEN_B, GEN_T)
    e_ref, e_off = rel_err(y_on.cpu().numpy(), ref.numpy()), rel_err(y_on.cpu().numpy(), y_off.cpu().numpy())
    print(case, "merged vs oracle %.3g, merged vs layer by layer %.3g, layer by layer vs oracle %.3g" % (e_ref, e_off, rel_err(y_off.cpu().numpy(), ref.numpy())))
    assert e_ref < ORACLE_TOL and e_off < FORWARD_TOL


# ------------------------------------------------------------------------------------------------ 2. ragged batches
def test_merged_ragged_batch():
    """Every utterance of a ragged batch (31, 13 and 0 frames) equals that utterance alone at its own length, with exact zeros past its end."""
    g, _ = build({"HIFICAR_MRF_MERGE": "2"})
    c, ar = gen_inputs()
    c, ar = c.cuda(), ar.cuda()
    with torch.no_grad():
        y, rows, _ = profiled(g, lambda: g(c, ar=ar, lengths=GEN_LENS))
        assert sorted(merged_rows(rows)) == sorted(expect_merged(GEN_PARAMS, [0, 1, 2]))
        for b, n in enumerate(GEN_LENS):
            assert float(y[b, :, GEN_HOP * n:].abs().sum()) == 0.0, b
            if n:
                alone, rows_1, _ = profiled(g, lambda: g(c[b:b + 1, :, :n].contiguous(), ar=ar[b:b + 1]))
                assert len(merged_rows(rows_1)) == 3
                assert same_across_shapes(y[b:b + 1, :, :GEN_HOP * n], alone, XSHAPE_TOL["f32"]), b


# ------------------------------------------------------------------------------------------------ 3. tile shapes
def merged_launch_layers(params, i):
    """The conv2 layers of stage i's last dilation, heaviest kernel first (what tile_admissible sees of the merged launch)."""
    C = _round_up(params["channels"] >> (i + 1), 32)
    return [Layer("convs2", C, params["channels"] >> (i + 1), k, 1, (k - 1) // 2) for k in sorted(params["resblock_kernel_sizes"], reverse=True)]


# name -> (model, batch, stages that must run merged, K chunks / 16 of their merged launches).  "wide": the small model at B = 24 — at B = 3 a launch
# the rule keeps from the forced shape (512-row tiles at a 64-channel chunk: upsamplers 0 and 1, stage 0) is planned freely and runs split-K, which
# rounds differently and would leave the forward comparable to a tolerance only; at B = 24 those launches fill the chip and the planner keeps them
# dense, which the test asserts by kernel name.  T = 31 keeps a partial last row tile at every tile height.  "narrow": stage widths 32 / 16 / 8 / 4, all
# padded to 32 channels: one 16-channel K chunk per slab (NC16 = 1, the one-slab-per-tap K loop), and every shape is admissible for every launch.
TILE_CASES = {"wide": (GEN_PARAMS, 24, {0, 1}, {2, 4}), "narrow": (NARROW_PARAMS, GEN_B, {0, 1, 2}, {1})}


@pytest.mark.parametrize("case", sorted(TILE_CASES))
def test_merged_output_does_not_depend_on_the_tile_shape(case):
    """Every dense exact-fp32 shape of the engine forced in turn (hificar_debug_force_tile applies to the merged launch as to any other; the
    register-blocked shapes do not exist in exact fp32).  By kernel name: the merged launch of a stage ran the forced instantiation exactly where
    tile_admissible lets it, and no launch of any forward ran a split-K form.  Dense forms accumulate in one order whatever the shape, the merged
    form included, so EVERY forced shape reproduces the first one's waveforms — a dense and a ragged batch — bit for bit."""
    params, B, must, chunks = TILE_CASES[case]
    g, _ = build({"HIFICAR_MRF_MERGE": "2"}, params)
    lib, eng = g._lib, g._lib.hificar_engine_of(g._native_handle())
    c, ar = gen_inputs(B)
    c, ar = c.cuda(), ar.cuda()
    lens = [max(0, GEN_T - 3 * (b % 12)) for b in range(B)] if B > GEN_B else GEN_LENS
    dense, forced_ran, base = [s for s in SHAPES if s[3] == 1 and s[4] == 1], set(), None
    assert len(dense) == 9
    for shape in dense:
        force(lib, eng, shape)
        try:
            with torch.no_grad():
                y, rows, _ = profiled(g, lambda: g(c, ar=ar))
                y_r, rows_r, _ = profiled(g, lambda: g(c, ar=ar, lengths=lens))
            torch.cuda.synchronize()
        finally:
            force(lib, eng, None)
        assert not [v[0] for v in list(rows.values()) + list(rows_r.values()) if v[0].startswith("conv_sk_")], (shape, rows)
        stages = {i for i, label in enumerate(expect_merged(params, [0, 1, 2])) if label in rows}
        assert stages >= must and sorted(merged_rows(rows)) == sorted(expect_merged(params, sorted(stages))) == sorted(merged_rows(rows_r)), sorted(rows)
        for i, label in zip(sorted(stages), expect_merged(params, sorted(stages))):
            ls = merged_launch_layers(params, i)
            name = "%s<%d,%d,%d,%d>" % (MRG, shape[0], shape[1], shape[2], ls[0].chunk // 16)
            if admissible("f32", shape, ls):
                assert rows[label][0] == name and rows_r[label][0] == name, (shape, label, rows[label])
                forced_ran.add(name)
            else:
                assert rows[label][0] != name, (shape, label)
        if base is None:
            base = (shape, y.cpu(), y_r.cpu())
        else:
            assert torch.equal(y.cpu(), base[1]) and torch.equal(y_r.cpu(), base[2]), (shape_id(shape), shape_id(base[0]))
    print(case, "forced merged instantiations:", sorted(forced_ran))
    assert {int(n.split("<")[1].split(",")[3][:-1]) for n in forced_ran} == chunks, sorted(forced_ran)
    assert len(forced_ran) >= (17 if case == "wide" else 9), sorted(forced_ran)


# ------------------------------------------------------------------------------------------------ 4. both tile walks
def test_merged_wide_batch_walks_several_positions_per_workgroup():
    """B = 24, T = 50 on the shipped model (as test_mrf_mean_folded_into_the_upsampler): stages 0 and 1 end in launch_conv launches (stage 2 runs the
    fused pair kernels, so it stays as it is).  With 32-row tiles forced a merged launch has more positions than the device has CUs, so workgroups
    walk several positions (three list entries each) one after the other; with the planner's shape, and in every other test of this file, a
    workgroup has one position or none.  Against the oracle and against the layer-by-layer model."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B, T = 24, 50
    g_on, sd = build({"HIFICAR_MRF_MERGE": "2"}, E2W_PARAMS)
    g_off, _ = build({"HIFICAR_MRF_MERGE": "0"}, E2W_PARAMS)
    x = torch.from_numpy(synth_features(B, T, 13, seed=783)).permute(0, 2, 1).contiguous().cuda()
    ar = torch.from_numpy(np.random.default_rng(783).uniform(-0.5, 0.5, (B, 1, 512)).astype(np.float32)).cuda()
    lib, eng = g_on._lib, g_on._lib.hificar_engine_of(g_on._native_handle())
    with torch.no_grad():
        y_off, rows_off, _ = profiled(g_off, lambda: g_off(x, ar=ar))
        ref = O.generator_forward(O.fold_weight_norm(sd), E2W_PARAMS, x[:4].cpu(), ar[:4].cpu())
        for shape in (None, (1, 1, 4, 1, 1)):
            force(lib, eng, shape)
            try:
                y_on, rows_on, _ = profiled(g_on, lambda: g_on(x, ar=ar))
                torch.cuda.synchronize()
            finally:
                force(lib, eng, None)
            check_forms(E2W_PARAMS, rows_on, rows_off, [0, 1], B, T)
            positions = []
            for i, label in enumerate(expect_merged(E2W_PARAMS, [0, 1])):
                mi, wm, wn, _ = map(int, re.match(MRG + r"<(\d+),(\d+),(\d+),(\d+)>", rows_on[label][0]).groups())
                rows_i = _round_up(T, 32) * int(np.prod(E2W_PARAMS["upsample_scales"][:i + 1]))
                positions.append(B * -(-rows_i // (32 * mi * wm)) * -(-(_round_up(E2W_PARAMS["channels"] >> (i + 1), 32) // 32) // wn))
            if shape:
                assert max(positions) > cus, (positions, cus)
            e_ref, e_off = rel_err(y_on[:4].cpu().numpy(), ref.numpy()), rel_err(y_on.cpu().numpy(), y_off.cpu().numpy())
            print("forced" if shape else "planned", "positions per merged launch", positions, "vs oracle %.3g, vs layer by layer %.3g" % (e_ref, e_off))
            assert e_ref < ORACLE_TOL and e_off < FORWARD_TOL


# ------------------------------------------------------------------------------------------------ 5. the AR loop
def test_merged_ar_loop_and_streaming_step():
    """ar_synthesis over three chunks (25 + 25 + a tail of 10 frames) with the merged form against without; twice with it: bit for bit; and a
    StreamingSynthesizer step launches the (kernel, launches) multiset of the offline step, merged launches included."""
    g_on, _ = build({"HIFICAR_MRF_MERGE": "2"})
    g_off, _ = build({"HIFICAR_MRF_MERGE": "0"})
    c, _ = gen_inputs(GEN_B, 60, seed=91)
    c = c.cuda()
    with torch.no_grad():
        g_on.profile_begin()
        y_on = g_on.ar_synthesis(c, 25)
        names = [s["name"] for s in g_on.profile_end()]
        assert sum(name.startswith(MRG) for name in names) >= 3 and not any(" x3" in name and ".convs2.2.1" in name and int(name.split("blocks.")[1].split(".")[0]) < 9
                                                                            for name in names), names
        y_again = g_on.ar_synthesis(c, 25)
        y_off = g_off.ar_synthesis(c, 25)
    assert y_on.shape == (GEN_B, 60 * GEN_HOP)
    assert torch.equal(y_on, y_again)
    assert same_across_shapes(y_on, y_off, XSHAPE_TOL["f32"])
    n = 3
    feats = torch.from_numpy(synth_features(n, 25, 13, seed=11)).cuda()
    st = StreamingSynthesizer(g_on, 25, max_sessions=8)
    sids = [st.open() for _ in range(n)]
    c1 = feats.permute(0, 2, 1).contiguous()
    with torch.no_grad():
        for k in range(2):  # the first round builds the launch shapes' schedules
            for b, sid in enumerate(sids):
                st.push(sid, feats[b])
            if k:
                g_on.profile_begin()
            st.step()
            if k:
                streamed = sorted((s["name"], s["launches"]) for s in g_on.profile_end())
            g_on.ar_synthesis(c1, 25)
        g_on.profile_begin()
        g_on.ar_synthesis(c1, 25)
        offline = sorted((s["name"], s["launches"]) for s in g_on.profile_end())
    assert streamed == offline
    assert sum(name.startswith(MRG) for name, _ in streamed) == 3, streamed


# ------------------------------------------------------------------------------------------------ 6. gating
@pytest.mark.parametrize("case", ["pair0", "ksplit0", "ksplit2", "tap", "train"])
def test_merged_form_is_off_where_a_path_is_pinned(case):
    """HIFICAR_PAIR=0 (layer by layer: no fused launch forms), HIFICAR_KSPLIT=0 (one accumulation order at every launch size), HIFICAR_KSPLIT=2 (every
    launch split-K: the merged form is dense), a registered debug tap
    (it wants the blocks' own outputs) and the forward under autograd (the tape keeps them): no merged launch even with HIFICAR_MRF_MERGE=2, and the
    waveform of the model built with HIFICAR_MRF_MERGE=0 bit for bit."""
    env = {"pair0": {"HIFICAR_PAIR": "0"}, "ksplit0": {"HIFICAR_KSPLIT": "0"}, "ksplit2": {"HIFICAR_KSPLIT": "2"}}.get(case, {})
    g_on, _ = build(dict(env, HIFICAR_MRF_MERGE="2"), remove_wn=case != "train")
    g_off, _ = build(dict(env, HIFICAR_MRF_MERGE="0"), remove_wn=case != "train")
    c, ar = gen_inputs()
    c, ar = c.cuda(), ar.cuda()

    def run(g):
        if case == "tap":
            with torch.no_grad():
                return g.debug_taps(["blocks.4"], c, ar=ar)[0]
        if case == "train":
            g.train()
            try:
                return g(c, ar=ar).detach()  # (gradients enabled: the taped forward)
            finally:
                g.eval()
        with torch.no_grad():
            return g(c, ar=ar)

    y_on, rows_on, others = profiled(g_on, lambda: run(g_on))
    y_off, rows_off, _ = profiled(g_off, lambda: run(g_off))
    assert rows_on and not merged_rows(rows_on) and not any(name.startswith(MRG) for name in others), sorted(rows_on)
    assert sorted((k, v[0], v[1]) for k, v in rows_on.items()) == sorted((k, v[0], v[1]) for k, v in rows_off.items())
    assert torch.equal(y_on, y_off)
    if case in ("pair0", "ksplit0", "ksplit2"):  # (and the switch alone does not turn the form off: without it the same model runs merged launches)
        g_free, _ = build({"HIFICAR_MRF_MERGE": "2"})
        with torch.no_grad():
            _, rows_free, _ = profiled(g_free, lambda: g_free(c, ar=ar))
        assert len(merged_rows(rows_free)) == 3
