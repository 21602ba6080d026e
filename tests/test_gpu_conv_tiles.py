"""Every tile shape of the conv engine, forced (hificar_debug_force_tile) and compared with the CPU oracle.  ``pytest -m gpu``.

The planner (pick_tile, csrc/hificar.hip) chooses one of 15 tile shapes (MI, WM, WN, KS, NB) per launch from a cost model, so a test of a
small model only ever runs the shapes small launches prefer.  Here every shape is forced in turn on models small enough for the oracle,
and every case asserts BY KERNEL NAME (profile rows with HIFICAR_PROFILE_DETAIL=1 carry the layer) that each launch ran the forced
instantiation wherever the engine's admissibility rule lets it, and did not where the rule forbids it.  The rule (tile_admissible in
csrc/hificar.hip) is restated below in ``admissible``; its inputs per launch are the layers' padded input width (-> K chunk), tap count,
halo, phases and 32-channel block count, which ``Layer`` derives as plan_layer does.

Instantiations built but admissible for NO layer of any model (LDS budget at zero halo: 2 x round_up(TM x chunk x 4, 1024) + out-buffer
<= 160 KiB; TM = 32 MI WM rows), from ``unreachable_instantiations`` and asserted by test_unreachable_instantiations_are_what_the_rule_says:
    exact fp32   conv_f32do_kernel<4,4,1,4>
    bf16x3       conv_bf16x3_kernel<4,4,1,2>, <4,2,2,4>, <4,4,1,4>, <2,4,1,4>;  conv_bf16x3nb_kernel<2,4,1,4>
Every other instantiation — 35 in exact fp32, 37 in bf16x3 — runs under force on the generator below (test_generator_reachable_set).

Bit identity: the dense forms (KS = 1, the register-blocked NB = 2 included) accumulate every output in one order whatever the tile shape, which
is what HIFICAR_KSPLIT=0 promises ("every launch shape uses one accumulation order").  The dense shapes are therefore forced on a model built
with HIFICAR_KSPLIT=0 — a launch the rule keeps from the forced shape then takes another DENSE shape — and must reproduce one dense shape's
taps, waveforms and gradients bit for bit; the split-K shapes run on a model with the default switch and agree to XSHAPE_TOL."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import E2W_PARAMS, rel_err
from articulatory_amd import _native
from articulatory_amd.models import HiFiGANGenerator, HiFiGANMultiScaleMultiPeriodDiscriminator
from articulatory_amd.utils.synth import synth_disc_state_dict, synth_features, synth_state_dict, uniform
from oracle import disc_oracle as DO
from oracle import hificar_oracle as O
from test_gpu_disc import SMALL_PERIOD, SMALL_SCALE
from test_gpu_parity import TOLS, XSHAPE_TOL

pytestmark = pytest.mark.gpu

# kTileCfgs of csrc/hificar.hip: (MI, WM, WN, KS, NB)
SHAPES = [(4, 1, 4, 1, 1), (4, 2, 2, 1, 1), (4, 4, 1, 1, 1), (2, 2, 2, 1, 2), (2, 4, 1, 1, 2), (2, 1, 4, 1, 2), (2, 1, 4, 1, 1), (2, 2, 2, 1, 1),
          (2, 4, 1, 1, 1), (1, 1, 4, 1, 1), (1, 2, 2, 1, 1), (1, 4, 1, 1, 1), (4, 1, 1, 4, 1), (2, 1, 1, 4, 1), (1, 1, 1, 4, 1)]
BASE_SHAPE = (2, 2, 2, 1, 1)  # the dense shape every other dense shape is compared with bit for bit (admissible for every launch here)
GRAD_TOL = 2e-4


def shape_id(s):
    return "mi%d_wm%d_wn%d_ks%d_nb%d" % s


def _round_up(x, m):
    return -(-x // m) * m


class Layer:
    """plan_layer of csrc/hificar.hip: what of a conv layer the tile rule reads."""

    def __init__(self, name, cin_pad, cout, K, dilation=1, padding=0, transposed=False, stride=1):
        self.name = name
        self.cin_pad = cin_pad
        cout_pad = _round_up(cout, 32)
        if not transposed:
            self.n_phase, self.ntaps = 1, K
            offs = [k * dilation - padding for k in range(K)]
        else:
            s = stride
            self.n_phase, self.ntaps = s, -(-K // s)
            offs = []
            for r in range(s):
                k0 = (r + padding) % s
                for t in range(self.ntaps):
                    assert (r + padding - (k0 + t * s)) % s == 0
                    offs.append((r + padding - (k0 + t * s)) // s)
        self.halo = max(0, max(offs)) - min(0, min(offs))
        self.chunk = 64 if cin_pad % 64 == 0 and cin_pad >= 128 else 32 if cin_pad % 32 == 0 and cin_pad >= 64 else 16
        self.n_blocks32 = cout_pad * self.n_phase // 32
        self.nb32_per_phase = cout_pad // 32


def out_buf_bytes(shape):
    mi, wm, wn, ks, nb = shape
    return ks * (wm * mi * 32) * (wn * nb * 32 + 4) * 4


def admissible(prec, shape, layers, ksplit=1):
    """tile_admissible of csrc/hificar.hip for a launch of these branches (layers[0] decides chunk and block count)."""
    mi, wm, wn, ks, nb = shape
    f32 = prec == "f32"
    L0 = layers[0]
    TM = wm * mi * 32
    halo = max(l.halo for l in layers)
    if nb == 2 and (f32 or L0.chunk == 16):
        return False  # not instantiated
    obuf = 0 if (f32 and ks == 1) else out_buf_bytes(shape)
    if 2 * _round_up((TM + halo) * L0.chunk * 4, 1024) + obuf > 160 * 1024:
        return False
    if nb == 2 and not (L0.n_blocks32 >= 2 and all(l.n_phase == 1 or l.nb32_per_phase % 2 == 0 for l in layers)):
        return False
    if ks == 4 and (ksplit == 0 or min(l.ntaps * (L0.chunk // 16) for l in layers) < 2):
        return False
    return True


def instantiation(prec, shape, chunk):
    """The kernel name (as the profile rows and rocprof print it) of a forced shape at a K chunk; None: no such instantiation is built."""
    mi, wm, wn, ks, nb = shape
    nc = chunk // 16
    if nb == 2 and (prec == "f32" or chunk == 16):
        return None
    if ks == 4:
        return "conv_sk_%s_kernel<%d,%d>" % ("f32" if prec == "f32" else "bf16x3", mi, nc)
    family = "conv_f32do_kernel" if prec == "f32" else "conv_bf16x3nb_kernel" if nb == 2 else "conv_bf16x3_kernel"
    return "%s<%d,%d,%d,%d>" % (family, mi, wm, wn, nc)


def n_tiles(shape, layers, nseq, rows, zrep=1):
    mi, wm, wn, ks, nb = shape
    return len(layers) * zrep * -(-layers[0].n_blocks32 // (wn * nb)) * nseq * -(-rows // (wm * mi * 32))


def unreachable_instantiations(prec):
    """Built instantiations (hificar_conv_inst.hip) that no launch can take whatever its layer: the rule at zero halo, one tap, even phases."""
    out = set()
    for shape in SHAPES:
        for chunk in (16, 32, 64):
            if instantiation(prec, shape, chunk) is None:
                continue
            free = Layer("x", {16: 32, 32: 64, 64: 128}[chunk], 64, 4 if shape[3] == 4 else 1, padding=0)
            free.halo = 0
            if not admissible(prec, shape, [free]):
                out.add(instantiation(prec, shape, chunk))
    return out


def test_unreachable_instantiations_are_what_the_rule_says():
    assert unreachable_instantiations("f32") == {"conv_f32do_kernel<4,4,1,4>"}
    assert unreachable_instantiations("bf16x3") == {"conv_bf16x3_kernel<4,4,1,2>", "conv_bf16x3_kernel<4,2,2,4>", "conv_bf16x3_kernel<4,4,1,4>",
                                                     "conv_bf16x3_kernel<2,4,1,4>", "conv_bf16x3nb_kernel<2,4,1,4>"}


# ------------------------------------------------------------------------------------------------ engine access
def force(lib, eng, shape):
    _native.check(lib.hificar_debug_force_tile(eng, *(shape if shape else (0, 0, 0, 0, 0))), "hificar_debug_force_tile")


def profile_rows(lib, eng):
    """{"layer xN": kernel} of the conv launches since hificar_profile_begin (HIFICAR_PROFILE_DETAIL=1 rows: "kernel|layer xN")."""
    stats, n = _native.profile_rows(lib, eng, 512)
    assert n <= 512
    rows = {}
    for name in (s["name"] for s in stats):
        if name.startswith("conv_") and "|" in name:
            kernel, layer = name.split("|")
            assert layer not in rows, (layer, kernel, rows[layer])  # one launch shape per layer in the profiled window
            rows[layer] = kernel
    return rows


def check_rows(rows, launches, prec, shape, ksplit=1):
    """Both directions: every launch the model makes is a profile row and vice versa; a launch runs the forced instantiation exactly
    where the rule admits it.  Returns the set of forced instantiations that ran."""
    want = {"%s x%d" % (ls[0].name, len(ls)): ls for ls, _ in launches}
    assert sorted(rows) == sorted(want)
    ran = set()
    for key, ls in want.items():
        forced = instantiation(prec, shape, ls[0].chunk)
        if admissible(prec, shape, ls, ksplit):
            assert rows[key] == forced, (key, rows[key], forced)
            ran.add(forced)
        else:
            assert rows[key] != forced, (key, forced)
    return ran


# ------------------------------------------------------------------------------------------------ (a), (b): the generator
# stage widths 192 / 96 / 48 / 24 -> row pitches 192 / 96 / 64 / 32 -> K chunks 64 / 32 / 32 / 16 and 6 / 3 / 2 / 1 channel blocks: a three-branch
# ResBlock launch at every chunk width, a partial channel group for WN = 4 (6 blocks) and WN = 2 (3 blocks); transposed layers at chunk 64
# (384 -> 192, 192 -> 96) and 32 (96 -> 48, 64 -> 24); the input conv (141 -> 144 input channels) at chunk 16
GEN_PARAMS = dict(E2W_PARAMS, channels=384, upsample_scales=[4, 2, 2, 2], upsample_kernel_sizes=[8, 4, 4, 4])
GEN_B, GEN_T, GEN_HOP = 3, 31, 32  # T <= 32: no bucket padding; 31 / 124 / 248 / 496 / 992 rows: a partial last tile at every tile height
GEN_LENS = [31, 13, 0]
GEN_SEED = 2024
TAPPED_BLOCKS = (0, 4, 8, 11)  # convs1.d / x.d of one block per stage (kernel sizes 3, 7, 11, 11)


def gen_launches(params, B, T, backward=False):
    """[([Layer of every branch, heaviest kernel first], rows)] of one forward (backward: of its data-gradient launches) with HIFICAR_PAIR=0."""
    ch, ks = params["channels"], params["kernel_size"]
    pad = lambda i: _round_up(ch >> i, 32)  # noqa: E731

    def conv(name, cin, cin_pad, cout, K, dil=1):  # a Conv1d with "same" padding, or its data gradient (make_dgrad_layer, csrc/hificar_train.hip.inc)
        p = (K - 1) // 2 * dil
        return Layer(name + "#dgrad", _round_up(cout, 32), cin, K, dil, (K - 1) * dil - p) if backward else Layer(name, cin_pad, cout, K, dil, p)

    out = [([conv("input_conv", params["in_channels"], max(32, _round_up(params["in_channels"], 16)), ch, ks)], T)]
    rows = T
    nb = len(params["resblock_kernel_sizes"])
    order = sorted(range(nb), key=lambda j: -params["resblock_kernel_sizes"][j])
    for i, (s, k) in enumerate(zip(params["upsample_scales"], params["upsample_kernel_sizes"])):
        name, p, C = "upsamples.%d.1" % i, s // 2 + s % 2, ch >> (i + 1)
        if backward:  # a Conv1d over the phase-major virtual channels of the output gradient
            jmin, jmax = (-p) // s, (k - 1 - p) // s
            out.append(([Layer(name + "#dgrad", _round_up(C, 32) * s, ch >> i, jmax - jmin + 1, padding=-jmin)], rows))
        else:
            out.append(([Layer(name, pad(i), C, k, transposed=True, stride=s, padding=p)], rows))
        rows *= s
        for d in range(len(params["resblock_dilations"][0])):
            for which in ("convs1", "convs2"):
                out.append(([conv("blocks.%d.%s.%d.1" % (i * nb + j, which, d), C, pad(i + 1), C, params["resblock_kernel_sizes"][j],
                                  params["resblock_dilations"][j][d] if which == "convs1" else 1) for j in order], rows))
    return out


def test_generator_model_meets_the_coverage_conditions():
    """From the test's own tile arithmetic: over the 15 shapes some forced launches have more tiles than the device has CUs (explicit LPT
    tile list) and some fewer (round-robin walk); every chunk width has a three-branch launch and a transposed layer; partial channel groups
    and partial row tiles occur."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    launches = gen_launches(GEN_PARAMS, GEN_B, GEN_T)
    assert {ls[0].chunk for ls, _ in launches if len(ls) == 3} == {16, 32, 64}
    assert {ls[0].chunk for ls, _ in launches if ls[0].n_phase > 1} == {32, 64}
    assert {ls[0].chunk for ls, _ in gen_launches(GEN_PARAMS, GEN_B, GEN_T, backward=True)} == {16, 32, 64}
    for prec in TOLS:
        more, fewer, part_group, part_rows = set(), set(), set(), set()
        for shape in SHAPES:
            for ls, rows in launches:
                if admissible(prec, shape, ls):
                    (more if n_tiles(shape, ls, GEN_B, rows) > cus else fewer).add(shape)
                    if ls[0].n_blocks32 % (shape[2] * shape[4]):
                        part_group.add(shape)
                    if rows % (shape[0] * shape[1] * 32):
                        part_rows.add(shape)
        assert more and fewer, (prec, cus, more, fewer)
        assert {s[2] * s[4] for s in part_group} >= {2, 4} and part_rows == {s for s in SHAPES if s[4] == 1 or prec != "f32"}


def test_generator_reachable_set():
    """The instantiations the generator cases below run under force, per arithmetic, from the rule alone (each case asserts its own part by
    kernel name): every built one except those no layer of any model can take (module docstring)."""
    for prec in TOLS:
        ran, built = set(), set()
        for shape in SHAPES:
            for chunk in (16, 32, 64):
                if instantiation(prec, shape, chunk) is not None:
                    built.add(instantiation(prec, shape, chunk))
            for ls, _ in gen_launches(GEN_PARAMS, GEN_B, GEN_T):
                if admissible(prec, shape, ls):
                    ran.add(instantiation(prec, shape, ls[0].chunk))
        assert len(built) == {"f32": 36, "bf16x3": 42}[prec]  # 9 x 3 dense + 9 split-K (+ 6 register-blocked)
        assert built - ran == unreachable_instantiations(prec), (prec, sorted(built - ran - unreachable_instantiations(prec)))


def _make_generator(prec, train=False):
    assert torch.cuda.is_available()
    sd = synth_state_dict(GEN_PARAMS, seed=1234)
    g = HiFiGANGenerator(**GEN_PARAMS, precision=prec)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    if train:
        return g.train().to("cuda:0"), sd
    g.remove_weight_norm()
    return g.eval().to("cuda:0"), sd


def _gen_inputs():
    c = torch.from_numpy(synth_features(GEN_B, GEN_T, 13, seed=GEN_SEED)).permute(0, 2, 1).contiguous()
    ar = torch.from_numpy(synth_features(GEN_B, 512, 1, seed=GEN_SEED + 1)[:, :, 0] * 0.3).reshape(GEN_B, 1, 512)
    return c, ar


TAP_NAMES = (["ar_feats", "input_conv"] + ["upsamples.%d" % i for i in range(4)] + ["blocks.%d" % n for n in range(12)]
             + ["blocks.%d.%s.%d" % (n, w, d) for n in TAPPED_BLOCKS for d in range(3) for w in ("convs1", "x")])
_GEN_ORACLE = {}


def _gen_oracle():
    """The CPU oracle's taps and waveform of the dense batch, and the waveform of every ragged utterance alone: once per module."""
    if not _GEN_ORACLE:
        w = O.fold_weight_norm(synth_state_dict(GEN_PARAMS, seed=1234))
        c, ar = _gen_inputs()
        slope = GEN_PARAMS["nonlinear_activation_params"]["negative_slope"]
        with torch.no_grad():
            taps = {}
            y = O.generator_forward(w, GEN_PARAMS, c, ar, taps=taps)
            want = {"ar_feats": taps["ar_feats"], "input_conv": taps["input_conv"]}
            for i in range(4):
                want["upsamples.%d" % i] = taps["upsample%d" % i]
            for n in range(12):
                want["blocks.%d" % n] = taps["blocks.%d" % n]
            for n in TAPPED_BLOCKS:  # residual_block.py:217-221, one layer at a time
                x, k = taps["upsample%d" % (n // 3)], GEN_PARAMS["resblock_kernel_sizes"][n % 3]
                for d, dil in enumerate(GEN_PARAMS["resblock_dilations"][n % 3]):
                    p1, p2 = "blocks.%d.convs1.%d.1" % (n, d), "blocks.%d.convs2.%d.1" % (n, d)
                    xt = F.conv1d(F.leaky_relu(x, slope), w[p1 + ".weight"], w[p1 + ".bias"], dilation=dil, padding=(k - 1) // 2 * dil)
                    want["blocks.%d.convs1.%d" % (n, d)] = xt
                    x = F.conv1d(F.leaky_relu(xt, slope), w[p2 + ".weight"], w[p2 + ".bias"], padding=(k - 1) // 2) + x
                    want["blocks.%d.x.%d" % (n, d)] = x
                assert torch.equal(x, taps["blocks.%d" % n])
            alone = [O.generator_forward(w, GEN_PARAMS, c[b:b + 1, :, :n], ar[b:b + 1]) if n else None for b, n in enumerate(GEN_LENS)]
        assert sorted(want) == sorted(TAP_NAMES)
        _GEN_ORACLE.update(y=y, taps=want, alone=alone)
    return _GEN_ORACLE


def _ksplit(shape):
    return 1 if shape[3] == 4 else 0  # the HIFICAR_KSPLIT of the model a shape is forced on (module docstring)


def _run_generator(g, shape):
    """One forced shape: taps + waveform, a plain forward (profiled), a ragged forward.  CPU tensors and the profile rows."""
    handle = g._native_handle()
    lib = g._lib
    eng = lib.hificar_engine_of(handle)
    c, ar = _gen_inputs()
    c, ar = c.cuda(), ar.cuda()
    force(lib, eng, shape)
    try:
        with torch.no_grad():
            y, taps = g.debug_taps(TAP_NAMES, c, ar=ar)
            _native.check(lib.hificar_profile_begin(eng), "hificar_profile_begin")
            y_plain = g(c, ar=ar)
            rows = profile_rows(lib, eng)
            y_ragged = g(c, ar=ar, lengths=GEN_LENS)
        torch.cuda.synchronize()
    finally:
        force(lib, eng, None)
    return dict(y=y.cpu(), y_plain=y_plain.cpu(), y_ragged=y_ragged.cpu(), taps={k: v.cpu() for k, v in taps.items()}), rows


@pytest.fixture(scope="module")
def detail_env():
    """HIFICAR_PAIR=0: the narrow stages go through launch_conv too; HIFICAR_PROFILE_DETAIL=1: profile rows carry the layer.  Both are read when
    a native handle is built, so they are set before any model of this module exists."""
    mp = pytest.MonkeyPatch()
    mp.setenv("HIFICAR_PAIR", "0")
    mp.setenv("HIFICAR_PROFILE_DETAIL", "1")
    mp.delenv("HIFICAR_KSPLIT", raising=False)
    yield mp
    mp.undo()


def _two_models(mp, make):
    """{HIFICAR_KSPLIT: model}: 0 for the dense shapes, the default (1) for the split-K shapes."""
    mp.setenv("HIFICAR_KSPLIT", "0")
    dense = make()
    dense._native_handle()  # (the switch is read when the native handle is built)
    mp.delenv("HIFICAR_KSPLIT")
    return {0: dense, 1: make()}


@pytest.fixture(scope="module", params=sorted(TOLS))
def gen(request, detail_env):
    """(arithmetic, {HIFICAR_KSPLIT: model}, results under BASE_SHAPE)."""
    prec = request.param
    models = _two_models(detail_env, lambda: _make_generator(prec)[0])
    launches = gen_launches(GEN_PARAMS, GEN_B, GEN_T)
    assert all(admissible(prec, BASE_SHAPE, ls, 0) for ls, _ in launches)
    base, rows = _run_generator(models[0], BASE_SHAPE)
    check_rows(rows, launches, prec, BASE_SHAPE, 0)
    return prec, models, base


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_generator_forward_forced_shape(gen, shape):
    """(a) every tap and the waveform against the oracle; a ragged batch, every utterance against the oracle on it alone and exact zeros
    past its end; dense shapes (KS = 1, NB = 2 included) bit-identical to each other, split-K shapes within XSHAPE_TOL of the dense result."""
    prec, models, base = gen
    tol = TOLS[prec]
    launches = gen_launches(GEN_PARAMS, GEN_B, GEN_T)
    got, rows = _run_generator(models[_ksplit(shape)], shape)
    ran = check_rows(rows, launches, prec, shape, _ksplit(shape))
    assert ran or (shape[4] == 2 and prec == "f32"), shape  # (NB = 2 does not exist in exact fp32: the planner's choice runs everywhere)
    ref = _gen_oracle()
    errs = {"waveform": rel_err(got["y"].numpy(), ref["y"].numpy()), "waveform (no taps)": rel_err(got["y_plain"].numpy(), ref["y"].numpy())}
    for name in TAP_NAMES:
        t = got["taps"][name]
        assert tuple(t.shape) == tuple(ref["taps"][name].shape) and bool(torch.isfinite(t).all()), name
        errs[name] = rel_err(t.numpy(), ref["taps"][name].numpy())
    for b, n in enumerate(GEN_LENS):
        assert float(got["y_ragged"][b, :, GEN_HOP * n:].abs().sum()) == 0.0, b
        if n:
            errs["ragged %d" % b] = rel_err(got["y_ragged"][b:b + 1, :, :GEN_HOP * n].numpy(), ref["alone"][b].numpy())
    xerr = max([rel_err(got[k].numpy(), base[k].numpy()) for k in ("y", "y_plain", "y_ragged")]
               + [rel_err(got["taps"][n].numpy(), base["taps"][n].numpy()) for n in TAP_NAMES])
    print(prec, shape_id(shape), "worst error vs oracle %.3g (%s), vs the dense base shape %.3g" % (max(errs.values()), max(errs, key=errs.get), xerr), sorted(ran))
    assert not {k: v for k, v in errs.items() if not v < tol}, {k: v for k, v in errs.items() if not v < tol}
    if shape[3] == 1:
        assert not any(k.startswith("conv_sk_") for k in rows.values()), rows  # every launch dense: one accumulation order
        for key in ("y", "y_plain", "y_ragged"):
            assert torch.equal(got[key], base[key]), key
        for name in TAP_NAMES:
            assert torch.equal(got["taps"][name], base["taps"][name]), name
    else:
        assert xerr < XSHAPE_TOL[prec], xerr


# LeakyReLU kinks: a pre-activation within rounding distance of zero flips between two correct fp32 computations and moves whole gradient tensors by
# percents.  Of seeds 0..39 the CPU oracle in fp32 and in fp64 agree on every tensor at twelve (to 3e-6); measured on the device with BASE_SHAPE, ten of
# those twelve flip a kink against the oracle (median tensor error 1e-6, a few tensors at 1e-2), seed 4 does not (worst tensor 3.1e-6 on the device,
# 2.7e-6 between the two CPU runs)
GRAD_SEED = 4
_GRAD = {}


def _grad_inputs():
    c_np = synth_features(GEN_B, GEN_T, 13, seed=GRAD_SEED).transpose(0, 2, 1).copy()
    ar_np = (synth_features(GEN_B, 512, 1, seed=GRAD_SEED + 1)[:, :, 0] * 0.4).reshape(GEN_B, 1, 512).astype(np.float32)
    cot = uniform(GRAD_SEED + 2, "cot", (GEN_B, 1, GEN_HOP * GEN_T), -1.0, 1.0)
    return c_np, ar_np, cot


def _run_backward(g, shape):
    handle = g._native_handle()
    lib = g._lib
    eng = lib.hificar_engine_of(handle)
    c_np, ar_np, cot = _grad_inputs()
    c = torch.from_numpy(c_np).cuda().requires_grad_(True)
    ar = torch.from_numpy(ar_np).cuda().requires_grad_(True)
    g.zero_grad(set_to_none=True)
    force(lib, eng, shape)
    try:
        _native.check(lib.hificar_profile_begin(eng), "hificar_profile_begin")
        y = g(c, ar=ar)
        (y * torch.from_numpy(cot).cuda()).sum().backward()
        torch.cuda.synchronize()
        rows = profile_rows(lib, eng)
    finally:
        force(lib, eng, None)
    got = {k: p.grad.detach().cpu().clone() for k, p in g.named_parameters()}
    got.update(c=c.grad.cpu(), ar=ar.grad.cpu(), y=y.detach().cpu())
    return got, rows


@pytest.fixture(scope="module")
def gen_train(detail_env):
    sd = synth_state_dict(GEN_PARAMS, seed=1234)
    models = _two_models(detail_env, lambda: _make_generator("f32", train=True)[0])
    base, _ = _run_backward(models[0], BASE_SHAPE)
    if not _GRAD:
        c_np, ar_np, cot = _grad_inputs()
        out, ref = O.gradients(sd, GEN_PARAMS, c_np, ar_np, cot)
        _GRAD.update(out=out, ref=ref)
    return models, base


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_generator_backward_forced_shape(gen_train, shape):
    """(b) train() mode, weight norm in the graph, exact fp32: every element of every gradient (parameters, c, ar) against the oracle's
    autograd; the forced instantiation ran in the forward AND in the data-gradient launches (mask_src / residual epilogue); dense shapes
    bit-identical; split-K shapes by the error-or-direction rule of test_gpu_disc_fuzz.py.  (Input seed: see GRAD_SEED.)"""
    models, base = gen_train
    ks = _ksplit(shape)
    bwd = gen_launches(GEN_PARAMS, GEN_B, GEN_T, backward=True)
    got, rows = _run_backward(models[ks], shape)
    ran = check_rows(rows, gen_launches(GEN_PARAMS, GEN_B, GEN_T) + bwd, "f32", shape, ks)
    if shape[4] == 1:  # (check_rows held every admitted launch to the forced instantiation: some of them are data-gradient launches)
        assert ran and any(admissible("f32", shape, ls, ks) for ls, _ in bwd)
    ref = _GRAD["ref"]
    assert rel_err(got["y"].numpy(), _GRAD["out"].numpy()) < 2e-5
    assert sorted(k for k in got if k != "y") == sorted(ref)
    dense = shape[3] == 1
    errs = {}
    for k in sorted(ref):
        a, b = got[k].double().reshape(-1), ref[k].double().reshape(-1)
        errs[k] = (float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)), 1.0 - float(a @ b / (a.norm() * b.norm()).clamp_min(1e-30)))
    worst = max(errs, key=lambda k: errs[k][0])
    print(shape_id(shape), "worst gradient error %.3g (1 - cos %.3g) in %s" % (errs[worst] + (worst,)), sorted(ran))
    bad = {k: v for k, v in errs.items() if not (v[0] < GRAD_TOL or (not dense and v[1] < 1e-5))}
    assert not bad, bad
    if dense:
        assert not any(k.startswith("conv_sk_") for k in rows.values()), rows
        for k in got:
            assert torch.equal(got[k], base[k]), k


# ------------------------------------------------------------------------------------------------ (c): the discriminators
DISC_PARAMS = dict(scales=2, scale_downsample_pooling="AvgPool1d", scale_downsample_pooling_params={"kernel_size": 4, "stride": 2, "padding": 2},
                   scale_discriminator_params=SMALL_SCALE, follow_official_norm=True, periods=[2, 3], period_discriminator_params=SMALL_PERIOD)
DISC_B, DISC_T = 2, 509
_DISC = {}


def disc_layers(cfg):
    """{profile-row layer name: Layer} of every ConvLayer disc_add_layer (csrc/hificar_disc.hip.inc) may build: the GEMM form over im2col rows
    (#g0), its data gradient (#g0#dgrad), the sliding-window polyphase form (#g0#poly) and its data gradient (#g0#polydgrad); the groups of a
    grouped conv are replicas of group 0's launch (zrep)."""
    out, groups = {}, {}

    def add(base, cin, cout, k, stride, g):
        cin_g, cout_g = cin // g, cout // g
        kg_pad, np_, ntp = _round_up(cin_g * k, 32), _round_up(cout_g, 32), -(-k // stride)
        for l in (Layer(base + "#g0", kg_pad, cout_g, 1), Layer(base + "#g0#dgrad", np_, kg_pad, 1),
                  Layer(base + "#g0#poly", stride * cin_g, cout_g, ntp), Layer(base + "#g0#polydgrad", np_, stride * cin_g, ntp, padding=ntp - 1)):
            out[l.name + " x1"] = l
            groups[l.name + " x1"] = g

    for i in range(cfg.n_scales):
        for l in range(cfg.s_n_layers):
            add("msd.discriminators.%d.layers.%d%s" % (i, l, ".0" if l + 1 < cfg.s_n_layers else ""), cfg.s_cin[l], cfg.s_cout[l], cfg.s_k[l],
                cfg.s_stride[l], cfg.s_groups[l])
    for i in range(cfg.n_periods):
        for l in range(cfg.p_n_layers):
            add("mpd.discriminators.%d%s" % (i, ".convs.%d.0" % l if l + 1 < cfg.p_n_layers else ".output_conv"), cfg.p_cin[l], cfg.p_cout[l],
                cfg.p_k[l], cfg.p_stride[l], 1)
    return out, groups


@pytest.fixture(scope="module")
def disc(detail_env):
    assert torch.cuda.is_available()
    sd = synth_disc_state_dict(DISC_PARAMS, seed=61)
    d = HiFiGANMultiScaleMultiPeriodDiscriminator(**DISC_PARAMS)
    assert list(d.state_dict()) == list(sd)
    d.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    d = d.to("cuda:0")
    if not _DISC:
        x_np = uniform(9, "x", (DISC_B, 1, DISC_T), -0.7, 0.7)
        with torch.no_grad():
            shapes = [[tuple(t.shape) for t in o] for o in d(torch.from_numpy(x_np).cuda())]
        cots = [[uniform(9, f"cot.{a}.{b}", s, -1.0, 1.0) / np.sqrt(np.prod(s[1:])) for b, s in enumerate(o)] for a, o in enumerate(shapes)]
        ref_outs, ref = DO.disc_gradients(sd, DISC_PARAMS, x_np, cots)
        assert shapes == [[tuple(t.shape) for t in o] for o in ref_outs]
        _DISC.update(x=x_np, cots=cots, outs=ref_outs, ref=ref)
    return d


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_discriminator_forced_shape(disc, shape):
    """(c) two scale discriminators (grouped layers: zrep > 1; strides 4) and periods 2, 3 (stride 3), B = 2, T = 509, the shape forced on the
    discriminators' engine: every layer output and every gradient against the oracle with the assertions of test_gpu_disc_fuzz.py, and by name
    the forced instantiation in every forward and data-gradient launch the rule admits."""
    d = disc
    handle = d._native_handle()
    lib = d._lib
    eng = lib.hificar_disc_engine(handle)
    layers, groups = disc_layers(d._config())
    x = torch.from_numpy(_DISC["x"]).cuda().requires_grad_(True)
    d.zero_grad(set_to_none=True)
    force(lib, eng, shape)
    try:
        _native.check(lib.hificar_profile_begin(eng), "hificar_profile_begin")
        outs = d(x)
        loss = 0.0
        for o, c in zip(outs, _DISC["cots"]):
            for t, ct in zip(o, c):
                loss = loss + (t * torch.from_numpy(ct).cuda()).sum()
        loss.backward()
        torch.cuda.synchronize()  # (the sub-discriminators run on side streams; profile_end waits for the last one used only)
        rows = profile_rows(lib, eng)
    finally:
        force(lib, eng, None)
    assert rows and set(rows) <= set(layers), sorted(set(rows) - set(layers))
    assert any(groups[k] > 1 for k in rows) and any("dgrad" in k for k in rows) and any("#poly " in k for k in rows)
    ran = set()
    for key, kernel in rows.items():
        forced = instantiation("f32", shape, layers[key].chunk)
        if admissible("f32", shape, [layers[key]]):
            assert kernel == forced, (key, kernel, forced)
            ran.add(forced)
        else:
            assert kernel != forced, (key, forced)
    assert ran or shape[4] == 2, shape
    print(shape_id(shape), sorted(ran))
    for o, r in zip(outs, _DISC["outs"]):
        for t, tr in zip(o, r):
            scale = float(tr.abs().max().clamp_min(1e-6))
            assert float((t.detach().cpu() - tr).abs().max()) < 2e-5 * scale
    got = {k: p.grad for k, p in d.named_parameters()}
    got["x"] = x.grad
    ref = _DISC["ref"]
    assert sorted(got) == sorted(ref)
    for k in ref:
        a, b = got[k].cpu().double().reshape(-1), ref[k].double().reshape(-1)
        err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
        cos = 1.0 - float(a @ b / (a.norm() * b.norm()).clamp_min(1e-30))
        assert err < 2e-4 or cos < 1e-5, (k, err, cos)
