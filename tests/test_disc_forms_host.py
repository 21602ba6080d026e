"""The discriminators' forms by arithmetic alone (CPU): the GPU cases of tests/test_gpu_disc_forms.py (tests/disc_forms.py: CASES) reach every
switch point of the table below; the cases the suite had before sit at none of them; and the window form's geometry holds for everything
hificar_disc_create accepts.  Everything here follows from the restated rule (tests/disc_forms.py); the GPU test asserts, by profile row,
that the device took the form the rule names."""
import os
import re

import numpy as np

import disc_forms as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "articulatory_amd", "csrc")


def _all_runs():
    return [(name, r) for name in F.CASES for r in F.case_runs(name)]


def test_restatement_quotes_the_source():
    """The conditions the rule restates, as the source writes them: a change there has to come here too."""
    inc = open(os.path.join(CSRC, "hificar_disc.hip.inc")).read()
    assert "L.can_window = !conv2d && !s.layers.empty() && k > 1 && L.cin_g % 4 == 0 && (stride * L.cin_g) % 32 == 0 && ntaps_p >= 2 && ntaps_p <= 11;" in inc
    assert "if (d->use_windows && L.can_window && s.layers[l - 1].cout_g % 4 == 0 && g.L[l + 1] >= d->window_min_rows) {" in inc
    assert "t.Lp = b.Lp = L.stride * (g.L[l + 1] + L.g[0].P.ntaps - 1);" in inc
    assert "int window_min_rows = %d;" % F.WINDOW_MIN_ROWS in inc and "bool use_windows = true;" in inc
    assert "return L + 2 * pad < k ? 0 : (L + 2 * pad - k) / stride + 1;" in inc
    assert "ip.src_mode == 2 && ip.cin_g % 4 == 0 && ip.prev_cout_g % 4 == 0" in inc
    assert "cp.np % 4 == 0 && cp.cout_g_prev % 4 == 0 && cp.cin_g % 4 == 0" in inc
    assert '"im2col_kernel|" + L.base + (vec4 ? " v4" : " v1")' in inc and '"col2im_mask_kernel|" + L.base + (vec4 ? " v4" : " v1")' in inc
    # neither switch of the window form can be set from outside: the cases reach both forms through T
    assert len(re.findall(r"use_windows", inc)) == 2 and len(re.findall(r"window_min_rows", inc)) == 2
    kern = open(os.path.join(CSRC, "hificar_disc_kernels.hip.h")).read()
    assert kern.count("if (p.win && t + p.win_off < p.win_rows) s +=") == 2  # both col2im kernels read a window row only where it exists
    assert "if (p.win) s +=" not in kern


def test_restated_stacks_are_the_package_s():
    from articulatory_amd.utils.synth import period_disc_layers, scale_disc_layers

    keys = ("cin", "cout", "k", "stride", "groups", "act", "bias", "pad")
    for name, (params, _, _) in list(F.CASES.items()) + [F.KINKED]:
        for mine, theirs in ((F.scale_layers("s", **params["scale_discriminator_params"]), scale_disc_layers(**params["scale_discriminator_params"])),
                             (F.period_layers("p", **params["period_discriminator_params"]), period_disc_layers(**params["period_discriminator_params"]))):
            assert [tuple(getattr(a, k) for k in keys) for a in mine] == [tuple(b[k] for k in keys) for b in theirs], name
    odd = F.layers_from_dicts("msd.discriminators.0", F.ODD_LAYERS)
    assert [l.base for l in odd] == ["msd.discriminators.0.layers.0.0", "msd.discriminators.0.layers.1.0", "msd.discriminators.0.layers.2"]


def test_cases_are_small():
    names = set()
    for name, (params, B, T) in list(F.CASES.items()) + [F.KINKED]:
        assert B <= 3 and F.admits(params, B, T), name
        runs = F.plan(params, B, T)
        assert max(max(r.layer.cin, r.layer.cout) for r in runs) <= 128, name
        assert sum(r.M * r.layer.cout * r.layer.cin_g * r.layer.k for r in runs) < 4e8, name  # multiply-accumulates of one forward
        assert len(runs) <= 24 and params["scales"] + len(params["periods"]) <= 8, name
        conv, gather, wgrad, _ = F.expected_rows(params, B, T)
        assert all(len("conv_f32do_kernel<4,1,4,4>|" + r) < 96 for r in list(conv) + list(gather)), name  # the name field of hificar_kernel_stat
        assert all(n == 1 for n in list(conv.values()) + list(gather.values())), name
        slopes = {params["scale_discriminator_params"]["nonlinear_activation_params"]["negative_slope"],
                  params["period_discriminator_params"]["nonlinear_activation_params"]["negative_slope"]}
        assert slopes == ({1.0} if name in F.CASES else {0.1, 1.0}), name
        names.add(name)
    assert F.KINKED[1][1:] == F.CASES["a_509"][1:]


def _conditions():
    """(what the issue's list asks for, does a case reach it): each from the rule's arithmetic over the cases' layers."""
    every = _all_runs()
    win = [(c, r) for c, r in every if r.window]
    im2 = [(c, r) for c, r in every if not r.window]
    strided_grouped = lambda r: r.layer.stride > 1 and r.layer.groups > 1  # noqa: E731
    shape = lambda r: (r.layer.cin, r.layer.cout, r.layer.k, r.layer.stride, r.layer.groups)  # noqa: E731
    at32 = {shape(r) for _, r in win if strided_grouped(r) and r.rows == 32}
    at31 = {shape(r) for _, r in im2 if strided_grouped(r) and r.layer.can_window and r.rows == 31}
    both_in_one_call = {(c, shape(r)) for c, r in win} & {(c, shape(r)) for c, r in im2 if r.layer.can_window}
    out = [
        ("one strided grouped layer shape: window at exactly 32 rows and im2col at 31 rows", bool(at32 & at31)),
        ("one layer definition in both forms in the same call", bool(both_in_one_call)),
        ("window layers with stride 1, 2 and 4", {r.layer.stride for _, r in win} >= {1, 2, 4}),
        ("window layers with 2 and 11 polyphase taps", {r.layer.ntaps for _, r in win} >= {2, 11}),
        ("k = 41 at stride 4 in the window form: 3 of 44 slots dropped", any(r.layer.k == 41 and r.layer.stride == 4 and r.layer.dropped_slots() == [41, 42, 43]
                                                                          for _, r in win)),
        ("two taps with one dropped slot", any(r.layer.ntaps == 2 and len(r.layer.dropped_slots()) == 1 for _, r in win)),
        ("more than 11 polyphase taps (k = 41, stride 2) stays im2col at window-sized rows",
         any(r.layer.k == 41 and r.layer.stride == 2 and r.layer.ntaps == 21 and not r.layer.can_window and r.rows >= F.WINDOW_MIN_ROWS
             and r.layer.cin_g % 4 == 0 and (r.layer.stride * r.layer.cin_g) % 32 == 0 for _, r in im2)),
        ("groups 1, 4 and 16", {r.layer.groups for _, r in every} >= {1, 4, 16}),
        ("groups 1, 4 and 16 in the window form", {r.layer.groups for _, r in win} >= {1, 4, 16}),
        ("a tail of stride - 1 unread padded input positions on a window layer", any(r.layer.stride > 1 and r.tail == r.layer.stride - 1 for _, r in win)),
        ("a tail of stride - 1 unread padded input positions on an im2col layer", any(r.layer.stride > 1 and r.tail == r.layer.stride - 1 and not r.layer.conv2d for _, r in im2)),
        ("scalar forward gather: cin_g no multiple of 4", any(r.prev is not None and r.layer.cin_g % 4 and r.prev.cout_g % 4 == 0 and not r.fwd_vec4 for _, r in every)),
        ("scalar forward gather: previous cout_g no multiple of 4", any(r.prev is not None and r.layer.cin_g % 4 == 0 and r.prev.cout_g % 4 and not r.fwd_vec4
                                                                       for _, r in every)),
        ("scalar col2im", any(r.col2im_vec4 is False for _, r in every)),
        ("4-wide gathers in both forms", {r.window for _, r in every if r.fwd_vec4} == {True, False}),
        ("4-wide col2im reading a window at exactly 32 rows", any(r.col2im_vec4 and r.next is not None and nr.window and nr.rows == 32
                                                                 for (_, r), (_, nr) in zip(every, every[1:]) if nr.sub is r.sub)),
        ("a window-capable layer refused the window only by the previous layer's cout_g", any(r.denied_by_prev for _, r in every)),
        ("stride-1 window layers at 32 and 33 rows, im2col at 16 and 17", {r.rows for _, r in win if r.layer.stride == 1} >= {32, 33}
         and {r.rows for _, r in im2 if r.layer.can_window and r.layer.stride == 1} >= {16, 17}),
    ]
    # pooled lengths, odd and even, under a pool other than (4, 2, 2)
    pooled = set()
    for name, (params, B, T) in F.CASES.items():
        if params["scale_downsample_pooling_params"] != F.POOL_422:
            pooled |= {r.L_in % 2 for r in F.plan(params, B, T) if r.sub.scale > 0 and r.l == 0}
    out.append(("odd and even pooled lengths under a pool other than AvgPool1d(4, 2, 2)", pooled == {0, 1}))
    # the period discriminators
    pc = [(name, params, B, T) for name, (params, B, T) in F.CASES.items() if params["periods"]]
    out.append(("periods [2, 3, 5, 7, 11]", bool(pc) and all(params["periods"] == [2, 3, 5, 7, 11] for _, params, _, _ in pc)))
    out.append(("a period stack whose channel count is no multiple of 4", any(params["period_discriminator_params"]["channels"] % 4 for _, params, _, _ in pc)))
    out.append(("narrow period stacks", all(params["period_discriminator_params"]["max_downsample_channels"] <= 32 for _, params, _, _ in pc)))
    for p in F.PERIODS:
        out.append(("period %d without reflect padding (T %% p = 0)" % p, any(T % p == 0 for _, _, _, T in pc)))
        out.append(("period %d with the maximal reflect padding (T %% p = 1)" % p, any(T % p == 1 and T > p for _, _, _, T in pc)))
    smallest = [T for _, params, B, T in pc if not F.admits(params, B, T - 1)]
    out.append(("the smallest T a period stack admits", bool(smallest)))
    out.append(("... with a layer stack on one row per column", any(r.L_in == 1 and r.l == 0 for name, _, _, T in pc if T in smallest for r in F.case_runs(name))))
    out.append(("T one above the reflect bound", any(T - 1 in smallest for _, _, _, T in pc)))
    return out


def test_cases_meet_the_coverage_conditions():
    missing = [what for what, ok in _conditions() if not ok]
    assert not missing, "no case reaches: " + "; ".join(missing)


def test_a_removed_case_is_noticed(monkeypatch):
    """The proof above is not vacuous: without the 32-row case, or without the refused-window case, it names what is lost."""
    for gone, lost in (("a_509", "window at exactly 32 rows and im2col at 31 rows"), ("f_150", "refused the window"), ("p8_6", "smallest T")):
        kept = F.OrderedDict((k, v) for k, v in F.CASES.items() if k != gone)
        monkeypatch.setattr(F, "CASES", kept)
        assert any(lost in what for what, ok in _conditions() if not ok), gone
        monkeypatch.undo()


def test_the_cases_the_suite_had_sit_at_no_switch_point():
    """test_gpu_disc.py's two configurations and the first 16 cases of test_gpu_disc_fuzz.py under the rule: the two configurations run window
    layers at 628 ... 33 rows, the fuzz at 43 rows or more; a window-capable layer takes the im2col form at 29 rows at most; none sits at 31 or
    32 rows.  (Why the cases of disc_forms.py exist.)"""
    from articulatory_amd.utils.synth import disc_params
    from test_disc_oracle import case_params
    from test_gpu_disc_fuzz import random_case

    golden = os.path.join(REPO, "tests", "golden")
    old = []
    for tag, T in (("small", 1031), ("default", 2512)):
        gold = np.load(os.path.join(golden, "gold_disc_%s.npz" % tag))
        assert int(gold["T"]) == T
        old.append((tag, disc_params(**case_params(tag)), int(gold["B"]), T))
    fuzz = [("fuzz%d" % i,) + (lambda c: (disc_params(**c[0]), c[1], c[2]))(random_case(i)) for i in range(16)]
    window_rows, fuzz_window_rows, im2col_rows, fuzz_im2col = set(), set(), set(), set()
    for name, params, B, T in old + fuzz:
        for r in F.plan(params, B, T):
            if r.window:
                (fuzz_window_rows if name.startswith("fuzz") else window_rows).add(r.rows)
            elif r.layer.can_window and r.prev.cout_g % 4 == 0:
                assert r.rows < F.WINDOW_MIN_ROWS
                (fuzz_im2col if name.startswith("fuzz") else im2col_rows).add(r.rows)
    assert sorted(window_rows, reverse=True) == [628, 315, 158, 157, 79, 65, 40, 33], sorted(window_rows)
    assert min(fuzz_window_rows) == 43 and max(fuzz_im2col) == 29 and max(im2col_rows) == 20, (sorted(fuzz_window_rows), sorted(fuzz_im2col), sorted(im2col_rows))
    assert not {31, 32} & (window_rows | fuzz_window_rows | im2col_rows | fuzz_im2col)


def test_window_geometry_over_everything_the_engine_accepts():
    """k 2..41, stride 1..8, pad 0..k-1, L_in k..k+3*stride+39, wherever the polyphase conv has 2..11 taps (hificar_disc_create accepts every
    one of them; the Python classes build odd k with pad (k - 1) / 2 only).
      every padded position the forward reads is < Lp:              holds
      every dropped polyphase slot has index >= k:                  holds
      every window row the col2im reads (t + pad, t < L_in) is < Lp: held for the geometries the Python classes build; failed for 10 407
          others (the smallest: k 4, stride 2, pad 0, L_in 5: Lp 4, row 4 read) until the kernels took the read under t + pad < Lp.  With that
          guard, restated in disc_forms.window_invariants: holds."""
    n = 0
    bad = {"forward": [], "col2im": [], "dropped": [], "col2im without the guard": []}
    for k in range(2, 42):
        for stride in range(1, 9):
            if not 2 <= -(-k // stride) <= F.MAX_WINDOW_TAPS:
                continue
            for pad in range(k):
                for L_in in range(k, k + 3 * stride + 40):
                    n += 1
                    f, c, d = F.window_invariants(k, stride, pad, L_in)
                    _, c0, _ = F.window_invariants(k, stride, pad, L_in, guarded=False)
                    for key, ok in (("forward", f), ("col2im", c), ("dropped", d), ("col2im without the guard", c0)):
                        if not ok:
                            bad[key].append((k, stride, pad, L_in))
                    if not c0:  # what the guard leaves out is a position no output reads: beyond the last one the forward touches
                        L_out, _, Lp = F.window_geometry(k, stride, pad, L_in)
                        assert stride * (L_out - 1) + k - 1 < Lp <= L_in - 1 + pad
    assert n == 284605
    assert not bad["forward"] and not bad["dropped"] and not bad["col2im"], {key: v[:3] for key, v in bad.items()}
    old = bad["col2im without the guard"]
    assert len(old) == 10407 and min(old, key=lambda g: g[3]) == (4, 2, 0, 5)
    assert not [g for g in old if g[0] % 2 == 1 and g[2] == (g[0] - 1) // 2]  # training through the package never was affected
    # the GPU case of this geometry
    runs = F.plan(F.ODD_PARAMS, F.ODD_B, F.ODD_T, scale_dicts=F.ODD_LAYERS)
    r = runs[1]
    assert r.window and r.rows >= F.WINDOW_MIN_ROWS and r.L_in + r.layer.pad > r.Lp and (r.layer.k, r.layer.stride, r.layer.pad) == (4, 2, 0)
    assert F.window_invariants(r.layer.k, r.layer.stride, r.layer.pad, r.L_in, guarded=False) == (True, False, True) and F.ODD_B == 3
    assert F.window_invariants(r.layer.k, r.layer.stride, r.layer.pad, r.L_in) == (True, True, True)
    assert F.plan(F.ODD_PARAMS, F.ODD_B, 2, scale_dicts=F.ODD_LAYERS)[1].M == 0  # T = 2 is too short for it: the call the GPU test expects to be refused


def test_the_unguarded_window_read_is_far_outside_the_bars():
    """Case (g) of the GPU test runs on the guarded kernels only.  What the read it guards against did, emulated in float64 on the CPU for that
    case's inputs: col2im added, at the last row of every sequence but the last, row 0 of the NEXT sequence's data gradient to dZ of layer 0 (for
    the last sequence it read past the group's piece: not emulated).  Through layer 0's transposed conv that moves dx by far more than the
    gradient bar: the element-wise comparison of (g) tells the two apart."""
    import pytest
    import torch
    import torch.nn.functional as TF

    import articulatory_amd.utils.synth as SY
    import test_gpu_disc_forms as G
    from oracle import disc_oracle as DO

    mp = pytest.MonkeyPatch()
    for mod in (SY, DO):
        mp.setattr(mod, "scale_disc_layers", lambda **_kw: [dict(L) for L in F.ODD_LAYERS])
    try:
        sd, x_np, cots = G.make_inputs(F.ODD_PARAMS, F.ODD_B, F.ODD_T, 7900)
    finally:
        mp.undo()
    w = {k: torch.from_numpy(v).double() for k, v in sd.items()}
    x = torch.from_numpy(x_np).double().requires_grad_(True)
    h, acts = x, []
    for l, L in enumerate(F.ODD_LAYERS):  # slope 1: the activations are the identity
        base = "msd.discriminators.0.layers.%d%s" % (l, ".0" if L["act"] else "")
        h = TF.conv1d(h, w[base + ".weight"], w[base + ".bias"], stride=L["stride"], padding=L["pad"], groups=L["groups"])
        h.retain_grad()
        acts.append(h)
    sum((a * torch.from_numpy(c).double()).sum() for a, c in zip(acts, cots[0])).backward()
    data_grad = acts[0].grad - torch.from_numpy(cots[0][0]).double()  # layer 1's data gradient with respect to its input, (B, 32, 69)
    assert float(data_grad[:, :, -1].abs().max()) == 0.0  # the last input row (pad 0, r = 1) is read by no output
    wrong = torch.zeros_like(data_grad)
    wrong[:-1, :, -1] = data_grad[1:, :, 0]
    dx_moved = TF.conv_transpose1d(wrong, w["msd.discriminators.0.layers.0.0.weight"], padding=F.ODD_LAYERS[0]["pad"])
    moved = float(dx_moved.abs().max() / x.grad.abs().max())
    assert moved > 100 * G.GRAD_TOL, moved
