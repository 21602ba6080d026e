"""Every form a discriminator layer can take, by name and element-wise against the float64 oracle, at the sizes where the form switches.
``pytest -m gpu``.

Per layer and per call the discriminators' engine chooses between the im2col GEMM form and the sliding-window (polyphase input) form — by the
layer's shape, the previous layer's width and the rows per sequence, hence by T — and between the scalar and the 4-wide gathers
(csrc/hificar_disc.hip.inc: disc_plan and the launchers).  tests/disc_forms.py restates that rule and lists twelve small configurations with T
(CASES) chosen from it; tests/test_disc_forms_host.py proves from the rule what they reach: one strided grouped layer shape in the window form at
exactly 32 rows and in the im2col form at 31, one layer definition in both forms in one call, window layers at stride 1, 2 and 4 with 2 .. 11
polyphase taps, 1, 4 and 16 groups, dropped polyphase slots, unread tails, the scalar gathers, the refused window, odd and even pooled lengths,
and the period form with no, maximal and near-total reflect padding.  Here each case, LeakyReLU slope 1 (the identity: no kinks; every form,
gather and reduction still runs — the mask is what the existing tests keep covering), one forward and backward of sum(out * cot) over every
layer output:
  (a) by name: with HIFICAR_PROFILE_DETAIL=1 the conv rows ("...|<layer>#g0 x1" against "#g0#poly", "#dgrad" against "#polydgrad") and the
      gather rows ("im2col_kernel|<layer> v4" / " v1", "col2im_mask_kernel|...") are exactly the rows the rule predicts, one launch each; the
      weight-gradient rows carry the predicted layer shapes (cout x K k1 over im2col rows, cout x stride cin k ntaps over window rows), their
      instantiations and split counts are read and printed, not predicted; the deferred reductions count every layer once.
  (b) element-wise, no direction clause: every element of every layer output within 2e-5 of its tensor's max (test_gpu_disc_fuzz.py) and of
      every gradient (every raw parameter, x) within 2e-4 (TOL of test_gpu_disc.py, GRAD_TOL of test_gpu_conv_tiles.py) of
      DO.disc_gradients(..., dtype=float64).
  (c) tails: a strided layer reads the padded positions 0 .. L_in + 2 pad - 1 - r only, r = (L_in + 2 pad - k) % stride.  For the cases with
      r = stride - 1 the float64 reference is computed again with those r positions cut off every such layer's padded input (real input rows
      where pad < r, as in the geometry of (g)): the same function, and the device matches it at the same bars.
  (d) one kinked run per form: config A at T = 509 with LeakyReLU(0.1); the input seed is the first of at most 6 whose float64 forward keeps
      every pre-activation further than 2e-6 of its tensor's scale from zero (measured on the CPU: seed 0 qualifies, margin 3.7e-6; seeds 1 and 5 would not); the same bars.
  (e) a second forward + backward on the same inputs, after the allocator's free blocks were filled with NaN, is bit-identical: the padded
      columns and the window buffers' padding rows are written, not assumed to be zero.
  (f) the cases that take a 4-wide gather are bit-identical under HIFICAR_COL2IM_VEC4=0 (a second module: the switch is read when the engine
      is created), and by name every gather then ran scalar — including the window read of col2im at exactly 32 rows.
  (g) a geometry hificar_disc_create accepts and the Python classes never build — k 4, stride 2, pad 0 on 69 rows: the window holds 68 rows, and
      row 68, which col2im read before it was guarded, is row 0 of the next sequence — through a test-local scale_disc_layers, B = 3, element-wise
      against F.conv1d in float64.  The same module first refuses a T too short for that layer (ValueError, before anything is enqueued).

The bars rest on the oracle's own arithmetic: its float32 run against its float64 run, on the CPU, over all cases, worst element relative to
the tensor's max (worst case named):
    layer outputs 8.0e-7 (a_509_kink); gradients of the parameters with more than one element 1.3e-6 (p6_2310), of x 5.3e-7 (d_150);
    one-element tensors: the scale output convs' biases 1.1e-6 (e_512), the period output convs' biases 1.5e-6 (p6_2310), the period output
    convs' weight_g 4.8e-5 (p8_2311; 2.4e-6 or less in the other period cases); the geometry of (g): outputs 3.5e-7, gradients 2.8e-7.
All but one are below a hundredth of their bar.  The period output conv's weight_g is one number, sum(dW * v) / |v|, a sum that cancels: the
oracle's own float32 run moves it by a quarter of the bar, so that tensor alone is held to the bar plus three times the measured gap,
2e-4 + 3 * 4.8e-5 = 3.44e-4 (ONE_ELEMENT_G_TOL)."""
from collections import Counter

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import disc_forms as F
from articulatory_amd import _native
from articulatory_amd.models import HiFiGANMultiScaleMultiPeriodDiscriminator
from articulatory_amd.utils.synth import synth_disc_state_dict, uniform
from oracle import disc_oracle as DO

pytestmark = pytest.mark.gpu
OUT_TOL = 2e-5
GRAD_TOL = 2e-4
KINK_MARGIN = 2e-6
SEEDS_TRIED = 6
ONE_ELEMENT_G_TOL = GRAD_TOL + 3 * 4.8e-5  # mpd.discriminators.<i>.output_conv.weight_g, one element (see the docstring)
ALL = list(F.CASES) + [F.KINKED[0]]
_INPUTS, _REF, _GOT = {}, {}, {}


def case_of(name):
    return F.CASES[name] if name in F.CASES else F.KINKED[1]


def case_seed(name):
    return 7300 + 10 * ALL.index(name)


def kink_margin(sd, params, x_np):
    """Smallest |x| / max|x| over every LeakyReLU input of the float64 oracle forward (slope-1 calls do not count)."""
    margins = []
    real = DO.F.leaky_relu

    def spy(x, negative_slope=0.01, *a, **kw):
        if negative_slope != 1.0 and x.numel():
            margins.append(float(x.abs().min() / x.abs().max().clamp_min(1e-300)))
        return real(x, negative_slope, *a, **kw)

    DO.F.leaky_relu = spy
    try:
        with torch.no_grad():
            DO.disc_forward(DO.fold_disc_weight_norm(sd, dtype=torch.float64), params, torch.from_numpy(x_np).double())
    finally:
        DO.F.leaky_relu = real
    return min(margins) if margins else 1.0


def make_inputs(params, B, T, seed, kinked=False):
    """(state dict, x, cotangents as in test_gpu_disc_fuzz.py): numpy, deterministic."""
    sd = synth_disc_state_dict(params, seed=seed)
    for attempt in range(SEEDS_TRIED if kinked else 1):
        x_np = uniform(seed + 1 + 1000 * attempt, "x", (B, 1, T), -0.7, 0.7)
        if not kinked or kink_margin(sd, params, x_np) > KINK_MARGIN:
            break
    else:
        pytest.fail("no input clear of the LeakyReLU kinks in %d seeds" % SEEDS_TRIED)
    with torch.no_grad():
        outs = DO.disc_forward(DO.fold_disc_weight_norm(sd, dtype=torch.float64), params, torch.from_numpy(x_np).double())
    shapes = [[tuple(t.shape) for t in o] for o in outs]
    cots = [[uniform(seed + 2, f"cot.{a}.{b}", s, -1.0, 1.0) / np.sqrt(np.prod(s[1:])) for b, s in enumerate(o)] for a, o in enumerate(shapes)]
    return sd, x_np, cots


def case_inputs(name):
    if name not in _INPUTS:
        params, B, T = case_of(name)
        _INPUTS[name] = make_inputs(params, B, T, case_seed(name), kinked=name == F.KINKED[0])
    return _INPUTS[name]


def case_reference(name):
    """The float64 oracle of a case, computed once: (layer outputs, gradients)."""
    if name not in _REF:
        sd, x_np, cots = case_inputs(name)
        _REF[name] = DO.disc_gradients(sd, case_of(name)[0], x_np, cots, dtype=torch.float64)
    return _REF[name]


@pytest.fixture(scope="module")
def detail_env():
    """HIFICAR_PROFILE_DETAIL=1: profile rows carry the layer and the gather's width.  Read when an engine is created, so it is set before
    any model of this module exists."""
    mp = pytest.MonkeyPatch()
    mp.setenv("HIFICAR_PROFILE_DETAIL", "1")
    mp.delenv("HIFICAR_COL2IM_VEC4", raising=False)
    yield mp
    mp.undo()


def build(params, sd):
    assert torch.cuda.is_available()
    d = HiFiGANMultiScaleMultiPeriodDiscriminator(**params)
    assert list(d.state_dict()) == list(sd)
    d.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return d.to("cuda:0")


def profile_rows(lib, eng):
    """{row: launches} since hificar_profile_begin."""
    rows, n = _native.profile_rows(lib, eng, 512)
    assert n <= 512
    return {r["name"]: r["launches"] for r in rows}


def step(d, x_np, cots, profile=False):
    """One forward and backward of sum(out * cot) over every layer output: (layer outputs, gradients of every parameter and x, profile rows)."""
    handle = d._native_handle()
    lib = d._lib
    eng = lib.hificar_disc_engine(handle)
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    d.zero_grad(set_to_none=True)
    rows = None
    if profile:
        _native.check(lib.hificar_profile_begin(eng), "hificar_profile_begin")
    try:
        outs = d(x)
        loss = 0.0
        for o, c in zip(outs, cots):
            for t, ct in zip(o, c):
                loss = loss + (t * torch.from_numpy(ct).cuda()).sum()
        loss.backward()
        torch.cuda.synchronize()  # (the sub-discriminators run on side streams; profile_end waits for the last one used only)
    finally:
        if profile:
            rows = profile_rows(lib, eng)
    got = {k: p.grad.detach().cpu().clone() for k, p in d.named_parameters()}
    got["x"] = x.grad.cpu()
    return [[t.detach().cpu() for t in o] for o in outs], got, rows


def check_rows(name, rows, expected):
    """(a): the profile's conv, gather and weight-gradient rows against the rule's, both ways.  Returns the lines to print."""
    conv_want, gather_want, wgrad_want, (n_w, n_b) = expected
    conv, gather, wgrad, ran = Counter(), Counter(), Counter(), []
    nw = nb = 0
    for row, count in rows.items():
        if row.startswith("conv_") and "|" in row:
            conv[row.split("|", 1)[1]] += count
        elif row.startswith(("im2col_kernel", "col2im_mask_kernel")):
            gather[row] += count
        elif row.startswith("wgrad_"):
            kernel, shape, split, rsplit, n = row.split(" ")
            assert split[0] == "s" and int(split[1:]) >= 1 and n == "n1", row
            wgrad[shape] += count
            ran.append(row)
        elif row.startswith("reduce_multi_kernel"):
            _, w, b = row.split(" ")
            nw, nb = nw + count * int(w[1:]), nb + count * int(b[1:])
    for what, got, want in (("conv", conv, conv_want), ("gather", gather, gather_want), ("weight gradient", wgrad, wgrad_want)):
        assert got == want, (name, what, sorted(set(got) - set(want)), sorted(set(want) - set(got)), {k: (got[k], want[k]) for k in set(got) & set(want) if got[k] != want[k]})
    assert (nw, nb) == (n_w, n_b), (name, nw, nb, n_w, n_b)
    assert not [r for r in rows if r.startswith(("wreduce", "breduce"))], sorted(rows)  # every reduction of a sub-discriminator's pass is deferred
    return sorted(ran)


def errors(outs, got, ref_outs, ref):
    """Worst element of every tensor relative to the reference tensor's max: ({(sub, layer): error}, {gradient: error})."""
    assert [[tuple(t.shape) for t in o] for o in outs] == [[tuple(t.shape) for t in o] for o in ref_outs]
    assert sorted(got) == sorted(ref)
    eo = {}
    for a, (o, r) in enumerate(zip(outs, ref_outs)):
        for b, (t, tr) in enumerate(zip(o, r)):
            assert bool(torch.isfinite(t).all()), (a, b)
            eo[(a, b)] = float((t.double() - tr.double()).abs().max() / tr.double().abs().max().clamp_min(1e-30))
    eg = {}
    for k in ref:
        assert tuple(got[k].shape) == tuple(ref[k].shape) and bool(torch.isfinite(got[k]).all()), k
        eg[k] = float((got[k].double() - ref[k].double()).abs().max() / ref[k].double().abs().max().clamp_min(1e-30))
    return eo, eg


def assert_close(name, outs, got, ref_outs, ref):
    """(b): every element, no tensor left out."""
    eo, eg = errors(outs, got, ref_outs, ref)
    wo = sorted(eo.items(), key=lambda kv: -kv[1])[:3]
    wg = sorted(eg.items(), key=lambda kv: -kv[1])[:4]
    print(name, "worst outputs %s; worst gradients %s" % (", ".join("%d.%d %.3g" % (k[0], k[1], v) for k, v in wo), ", ".join("%s %.3g" % kv for kv in wg)))
    assert wo[0][1] < OUT_TOL, (name, wo)
    bad = {k: v for k, v in eg.items() if not v < (ONE_ELEMENT_G_TOL if k.endswith(".output_conv.weight_g") and ref[k].numel() == 1 else GRAD_TOL)}
    assert not bad, (name, sorted(bad.items(), key=lambda kv: -kv[1]))


def case_results(name):
    """The device's results of a case (a module built under the detail switch), computed once: (outputs, gradients, profile rows) of a first
    forward + backward and (outputs, gradients) of a second one on dirty scratch."""
    if name not in _GOT:
        params, B, T = case_of(name)
        sd, x_np, cots = case_inputs(name)
        d = build(params, sd)
        if params["periods"] and not F.admits(params, B, T - 1):  # one sample fewer than the stacks admit: refused, and the module works on
            with pytest.raises(ValueError, match="reflect padding"):
                d(torch.zeros(B, 1, T - 1, device="cuda"))
        first = step(d, x_np, cots, profile=True)
        torch.empty(1 << 24, device="cuda").fill_(float("nan"))  # poison the allocator's free blocks: stale memory must not pass as zeros
        _GOT[name] = first + step(d, x_np, cots)[:2]
    return _GOT[name]


@pytest.mark.parametrize("name", ALL)
def test_disc_forms_case(detail_env, name):
    params, B, T = case_of(name)
    sd, x_np, cots = case_inputs(name)
    outs, got, rows, outs2, got2 = case_results(name)
    ran = check_rows(name, rows, F.expected_rows(params, B, T))
    runs = F.plan(params, B, T)
    print(name, "window: %s" % ", ".join("%s@%d" % (r.layer.base.split("discriminators.")[1], r.rows) for r in runs if r.window))
    print("   ", "\n    ".join(ran))
    forms = {r.split(" ")[1].split("k")[1] == "1p1" for r in ran}  # one tap over im2col rows / all taps over window rows
    assert forms == {not r.window for r in runs}, (name, ran)
    ref_outs, ref = case_reference(name)
    assert_close(name, outs, got, ref_outs, ref)
    # (e) again, on dirty scratch
    for o, o2 in zip(outs, outs2):
        for t, t2 in zip(o, o2):
            assert torch.equal(t, t2), name
    for k in got:
        assert torch.equal(got[k], got2[k]), (name, k)


def test_cases_reach_both_weight_gradient_forms(detail_env):
    """Over the cases, the one-tap launch over im2col rows and the all-taps launch over window rows both occur, the latter at 2, 3, 5 and 11 taps."""
    taps = set()
    for name in ("a_509", "c_140"):
        rows = case_results(name)[2]
        taps |= {int(r.split(" ")[1].split("k")[1].split("p")[0]) for r in rows if r.startswith("wgrad_")}
    assert taps >= {1, 2, 3, 5, 11}, taps


# ------------------------------------------------------------------------------------------------ (c) tails
def tail_layers(runs):
    """{(scale, layer): r} of the strided scale-discriminator layers whose last r = stride - 1 padded input positions no output reads."""
    return {(r.sub.scale, r.l): r.tail for r in runs if r.sub.period == 0 and r.layer.stride > 1 and r.tail == r.layer.stride - 1}


def gradients_without_tails(sd, params, x_np, cots, cut, layer_dicts=None):
    """DO.disc_gradients in float64 for scale discriminators only, every layer in ``cut`` run on its explicitly padded input WITHOUT the last
    cut[(scale, layer)] padded positions (conv1d with padding 0)."""
    from articulatory_amd.utils.synth import scale_disc_layers

    assert not params["periods"]
    leaves = {k: torch.as_tensor(np.asarray(v)).double().clone().requires_grad_(True) for k, v in sd.items()}
    x = torch.from_numpy(x_np).double().requires_grad_(True)
    layers = layer_dicts or scale_disc_layers(**params["scale_discriminator_params"])
    slope = params["scale_discriminator_params"]["nonlinear_activation_params"]["negative_slope"]
    pool = params["scale_downsample_pooling_params"]
    outs, xs = [], x
    for i in range(params["scales"]):
        h, o = xs, []
        for l, L in enumerate(layers):
            base = f"msd.discriminators.{i}.layers.{l}" + (".0" if L["act"] else "")
            h = TF.pad(h, (L["pad"], L["pad"]))
            if (i, l) in cut:
                h = h[..., : h.shape[-1] - cut[(i, l)]]
            h = TF.conv1d(h, leaves[base + ".weight"], leaves.get(base + ".bias"), stride=L["stride"], padding=0, groups=L["groups"])
            if L["act"]:
                h = TF.leaky_relu(h, slope)
            o.append(h)
        outs.append(o)
        xs = TF.avg_pool1d(xs, pool["kernel_size"], pool["stride"], pool["padding"])
    loss = 0.0
    for o, c in zip(outs, cots):
        for a, b in zip(o, c):
            loss = loss + (a * torch.from_numpy(np.asarray(b)).double()).sum()
    loss.backward()
    grads = {k: v.grad for k, v in leaves.items()}
    grads["x"] = x.grad
    return [[t.detach() for t in o] for o in outs], grads


TAIL_CASES = [n for n in F.CASES if tail_layers(F.case_runs(n))]


@pytest.mark.parametrize("name", TAIL_CASES)
def test_unread_tail_contributes_nothing(detail_env, name):
    params, B, T = case_of(name)
    runs = F.plan(params, B, T)
    cut = tail_layers(runs)
    assert cut and {r.window for r in runs if (r.sub.scale, r.l) in cut}  # (the host test proves: between the cases, both forms)
    sd, x_np, cots = case_inputs(name)
    cut_outs, cut_ref = gradients_without_tails(sd, params, x_np, cots, cut)
    ref_outs, ref = case_reference(name)
    eo, eg = errors(cut_outs, cut_ref, ref_outs, ref)  # the same function: float64 rounding apart
    assert max(eo.values()) < 1e-12 and max(eg.values()) < 1e-12, (name, max(eo.values()), max(eg.values()))
    outs, got = case_results(name)[:2]
    assert_close(name + " without its tails %s" % sorted(cut.items()), outs, got, cut_outs, cut_ref)


# ------------------------------------------------------------------------------------------------ (f) scalar against 4-wide
VEC4_CASES = [n for n in F.CASES if any(r.fwd_vec4 or r.col2im_vec4 for r in F.case_runs(n))]


@pytest.mark.parametrize("name", VEC4_CASES)
def test_scalar_gathers_are_bit_identical(detail_env, name):
    params, B, T = case_of(name)
    sd, x_np, cots = case_inputs(name)
    outs, got, rows = case_results(name)[:3]
    assert any(r.endswith(" v4") for r in rows), name
    detail_env.setenv("HIFICAR_COL2IM_VEC4", "0")  # read when the engine is created
    try:
        d0 = build(params, sd)
        outs0, got0, rows0 = step(d0, x_np, cots, profile=True)
    finally:
        detail_env.delenv("HIFICAR_COL2IM_VEC4")
    check_rows(name, rows0, F.expected_rows(params, B, T, vec4_enabled=False))
    assert not any(r.endswith(" v4") for r in rows0), sorted(rows0)
    for o, o0 in zip(outs, outs0):
        for t, t0 in zip(o, o0):
            assert torch.equal(t, t0), name
    for k in got:
        assert torch.equal(got[k], got0[k]), (name, k)


# ------------------------------------------------------------------------------------------------ (g) the window shorter than its input
def test_window_shorter_than_the_input(detail_env):
    import articulatory_amd.models.discriminator as MD
    import articulatory_amd.utils.synth as SY

    params, B, T = F.ODD_PARAMS, F.ODD_B, F.ODD_T
    layers = lambda **_kw: [dict(L) for L in F.ODD_LAYERS]  # noqa: E731
    mp = pytest.MonkeyPatch()
    for mod in (MD, SY, DO):  # the module, the synthetic state dict and the oracle all take the stack from this function
        mp.setattr(mod, "scale_disc_layers", layers)
    try:
        runs = F.plan(params, B, T, scale_dicts=F.ODD_LAYERS)
        assert runs[1].window and runs[1].L_in + runs[1].layer.pad > runs[1].Lp
        sd, x_np, cots = make_inputs(params, B, T, 7900)
        d = build(params, sd)
        with pytest.raises(ValueError, match="too short"):  # T = 2: layer 1 (k = 4, no padding) has no output row
            d(torch.zeros(B, 1, 2, device="cuda"))
        outs, got, rows = step(d, x_np, cots, profile=True)
        ran = check_rows("odd", rows, F.expected_rows(params, B, T, scale_dicts=F.ODD_LAYERS))
        print("   ", "\n    ".join(ran))
        assert "col2im_mask_kernel|msd.discriminators.0.layers.0.0 v4" in rows and any(r.endswith("layers.1.0#g0#polydgrad x1") for r in rows)
        ref_outs, ref = DO.disc_gradients(sd, params, x_np, cots, dtype=torch.float64)
        assert_close("odd", outs, got, ref_outs, ref)
        # (c) here on real input rows: layer 1's last input row (pad 0, r = 1) is read by no output
        cut = tail_layers(runs)
        assert cut == {(0, 1): 1}
        cut_outs, cut_ref = gradients_without_tails(sd, params, x_np, cots, cut, layer_dicts=F.ODD_LAYERS)
        assert_close("odd without its tail", outs, got, cut_outs, cut_ref)
        detail_env.setenv("HIFICAR_COL2IM_VEC4", "0")  # ... and through the scalar col2im
        try:
            d0 = build(params, sd)
            outs0, got0, rows0 = step(d0, x_np, cots, profile=True)
        finally:
            detail_env.delenv("HIFICAR_COL2IM_VEC4")
        assert "col2im_mask_kernel|msd.discriminators.0.layers.0.0 v1" in rows0
        for k in got:
            assert torch.equal(got[k], got0[k]), k
    finally:
        mp.undo()
