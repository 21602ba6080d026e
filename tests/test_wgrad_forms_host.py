"""The weight-gradient family by arithmetic alone (CPU): the instantiations the library builds, read from the dispatch's text; the GPU cases
of tests/test_gpu_wgrad_forms.py (tests/wgrad_forms.py: CASES) reach every one of them; and between them the cases contain every condition
of the table below.  Everything here follows from the restated rule (tests/wgrad_forms.py); the GPU test asserts, by kernel name, that the
device took the form the rule names.

Built instantiations that no case reaches (``UNREACHED``): none.

Reductions: the generator's backward defers every weight / bias reduction of a pass to reduce_multi_kernel (hificar_backward_cond sets
BwdWs::defer), so wreduce_kernel and breduce_kernel as launches of their own are not reachable through the generator; the discriminators, the
BiGRU and the Transformer take them (not this test's subject)."""
import os
import re

import wgrad_forms as W

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_INC = os.path.join(REPO, "articulatory_amd", "csrc", "hificar_train.hip.inc")
UNREACHED = set()


def _all_launches():
    return [(name, l) for name in W.CASES for l in W.case_launches(name)]


def _taps(launches):
    return [(c, l) for c, l in launches if l.kernel.startswith("wgrad_taps_kernel")]


def test_built_set_is_what_the_dispatch_instantiates():
    """The written-out set (wgrad_forms.BUILT) against the HIFICAR_WGT switch of launch_wgrad_n, the GEMM launches and wgrad_setup's list."""
    assert len(W.BUILT) == 2 * (5 + 2) + 5 + 2 + 1
    src = open(TRAIN_INC).read()
    body = src[src.index("static int launch_wgrad_n("):src.index("static int launch_wgrad(")]
    # the macro: R = 32 and 64 take <NT, EX, R>, R = 128 takes <min(NT, 7), EX, 128>
    assert "if (cr == 32) HIFICAR_WGT1(NT, EX, 32);" in body and "else if (cr == 128) HIFICAR_WGT1((NT <= 7 ? NT : 7), EX, 128);" in body
    assert "else HIFICAR_WGT1(NT, EX, 64);" in body and "wgrad_taps_kernel<NT, EX, R>" in body
    switch = body[body.index("switch (L.ntaps)"):body.index("#undef HIFICAR_WGT")]
    calls = [(int(nt), ex == "true") for nt, ex in re.findall(r"HIFICAR_WGT\((\d+), (true|false)\)", switch)]
    assert len(calls) == len(set(calls)) == 7
    assert (3, False) not in calls
    # an exact form is selected by its own case label, an inexact one only in the default arm
    exact = sorted(nt for nt, ex in calls if ex)
    assert exact == [1, 2, 3, 7, 11] and all(("case %d: HIFICAR_WGT(%d, true); break;" % (nt, nt)) in switch for nt in exact)
    assert len(re.findall(r"case \d+:", switch)) == len(exact)
    assert re.search(r"default:\s*if \(L\.ntaps < 7\) HIFICAR_WGT\(7, false\);\s*else HIFICAR_WGT\(11, false\);", switch)
    built = set()
    for nt, ex in calls:
        built |= {"wgrad_taps_kernel<%d,%d,%d>" % (nt, ex, r) for r in (32, 64)} | {"wgrad_taps_kernel<%d,%d,128>" % (min(nt, 7), ex)}
    built |= {"wgrad_gemm_kernel<%s,%s>" % m for m in re.findall(r"HIFICAR_WGG\((\d+), (\d+),", body)}
    assert "hipLaunchKernelGGL(wgrad_kernel," in body
    built.add("wgrad_kernel")
    assert built == set(W.BUILT), (sorted(built - W.BUILT), sorted(W.BUILT - built))
    # wgrad_setup raises the LDS limit of exactly the taps forms the switch can launch
    setup = src[src.index("static int wgrad_setup()"):src.index("static void train_free_impl")]
    lds = [(int(nt), ex == "true") for nt, ex in re.findall(r"HIFICAR_WGT_LDS\((\d+), (true|false)\);", setup)]
    assert sorted(lds) == sorted(calls)
    # the NT / EXACT rule of the restatement names, for every tap count and chunk, a built instantiation
    for ntaps in range(1, W.MAX_TAPS_ALL + 1):
        for cr in (32, 64) + ((128,) if ntaps <= 7 else ()):
            assert W.taps_instantiation(ntaps, cr) in W.BUILT


def test_cases_reach_every_built_instantiation():
    reached = {l.kernel for _, l in _all_launches()}
    assert reached <= W.BUILT
    assert W.BUILT - reached == UNREACHED, sorted(W.BUILT - reached - UNREACHED)


def test_cases_are_small():
    """One or two stages, B = 3, a few thousand output samples at most, at most 64 reductions per pass (one reduce_multi_kernel launch)."""
    assert W.B == 3
    for name, (params, T) in W.CASES.items():
        hop = 1
        for s in params["upsample_scales"]:
            hop *= s
        assert len(params["upsample_scales"]) in (1, 2) and W.B * T * hop <= 4000, name
        assert len(W.case_launches(name)) < 64, name
        assert all(len(l.row()) + len(" s256") < 96 for l in W.case_launches(name)), name  # the name field of hificar_kernel_stat
        assert params["nonlinear_activation_params"] == {"negative_slope": 1.0}


def test_cases_meet_the_coverage_conditions():
    """The table of conditions, each from the rule's arithmetic over the cases' launches."""
    every = _all_launches()
    taps = _taps(every)
    pertap = [(c, l) for c, l in every if l.kernel == "wgrad_kernel"]
    gemm = [(c, l) for c, l in every if l.kernel.startswith("wgrad_gemm_kernel")]
    # wgrad_kernel at row_split 1, 2 and 4; rows no multiple of its 128-row chunk and more than one chunk per sequence, at row_split 1 and 4
    assert {l.row_split for _, l in pertap} == {1, 2, 4}
    assert {l.row_split for _, l in pertap if l.rows > 128 and l.rows % 128} >= {1, 4}
    assert any(l.rows < 128 for _, l in pertap)  # ... and a single, partly filled chunk
    assert {l.L.ntaps for _, l in pertap} >= {13, 15}
    # the taps forms: NT 1, 2, 3, 7, 11 exact and 7, 11 inexact at R = 32 and R = 64; NT 1, 2, 3, 7 exact and 7 inexact at R = 128
    kernels = {l.kernel for _, l in taps}
    for r in (32, 64):
        assert kernels >= {"wgrad_taps_kernel<%d,1,%d>" % (nt, r) for nt in (1, 2, 3, 7, 11)} | {"wgrad_taps_kernel<%d,0,%d>" % (nt, r) for nt in (7, 11)}
    assert kernels >= {"wgrad_taps_kernel<%d,1,128>" % nt for nt in (1, 2, 3, 7)} | {"wgrad_taps_kernel<7,0,128>"}
    # R = 64 for each of its three reasons: 33..64 rows, more than 7 taps over long sequences, a halo above 32 rows
    r64 = [l for _, l in taps if l.chunk == 64]
    assert any(32 < l.rows <= 64 for l in r64) and any(l.L.ntaps > 7 and l.rows > 64 for l in r64)
    assert any(l.L.ntaps <= 7 and l.rows > 64 and l.L.halo > 32 for l in r64)
    # rows no multiple of R, the last chunk partly past the sequence end, with B > 1: every R; and more than one chunk per sequence where
    # the rule allows it (R = 32 is only chosen for sequences of at most 32 rows)
    for r in (32, 64, 128):
        assert any(l.chunk == r and l.rows % r for _, l in taps), r
    for r in (64, 128):
        assert any(l.chunk == r and l.rows % r and l.rows > r for _, l in taps), r
    assert all(l.rows % l.chunk for _, l in gemm)
    # a halo larger than the chunk (kernel 11, dilation 5 at R = 32)
    assert any(l.chunk == 32 and max(x.halo for x in l.layers) > 32 for _, l in taps)
    # row_split 2 and 4 in the taps kernel, the latter at R = 64 and R = 128; can32 false: at most 32 rows, yet R = 64
    assert {l.row_split for _, l in taps} == {1, 2, 4}
    assert {l.chunk for _, l in taps if l.row_split == 4} == {64, 128}
    assert any(l.row_split == 4 and l.rows <= 32 and l.chunk == 64 for _, l in taps)
    # g_per_tile = 1 at odd and even scales, at row_split 2 and 4
    gpt1 = [l for _, l in taps if l.g_per_tile == 1]
    assert {l.L.n_phase % 2 for l in gpt1} == {0, 1} and {l.row_split for l in gpt1} == {2, 4}
    assert all(l.L.n_phase > 1 and l.L.nb32_per_phase % 2 == 1 for l in gpt1)
    # a partial 32-block of A (pitch a multiple of 16 only): in the taps kernel, the per-tap kernel and the 128 x 128 GEMM tile
    for group in (taps, pertap, [(c, l) for c, l in gemm if l.kernel == "wgrad_gemm_kernel<2,64>"]):
        assert any(l.L.cin_pad % 32 == 16 for _, l in group)
    # output widths that are no multiple of 32
    assert {l.L.cout for _, l in every} >= {24, 48, 100}
    # paired and single launches of the same layer shape in the same instantiation
    both = {(l.kernel, l.L.shape()) for _, l in taps if l.n == 2} & {(l.kernel, l.L.shape()) for _, l in taps if l.n == 1 and not l.unpaired}
    assert len({k for k, _ in both}) >= 4, both
    # pairs that fall back to two singles: more than 11 taps, and unlike chunk rows
    assert any(l.unpaired and l.kernel == "wgrad_kernel" for _, l in every)
    assert {l.chunk for _, l in taps if l.unpaired} == {64, 128}
    # the GEMM forms: <2,64> with a partial tile of A (its blocks no multiple of the tile's four), <4,32>; both as input conv and as ResBlock
    assert any(l.kernel == "wgrad_gemm_kernel<2,64>" and l.L.n_ablk % 4 for _, l in gemm)
    for k in ("wgrad_gemm_kernel<2,64>", "wgrad_gemm_kernel<4,32>"):
        assert {l.L.name == "input_conv" for _, l in gemm if l.kernel == k} == {True, False}, k
    # paired one-tap layers at least 128 wide: the taps kernel runs, the split comes from the GEMM branch of wgrad_split
    assert any(l.n == 2 and W.wgrad_gemm_form(l.L) and l.kernel.startswith("wgrad_taps_kernel<1,1,") for _, l in taps)
    # layers with and without bias
    assert {l.bias for _, l in taps} == {True, False} and any(not l.bias for _, l in taps if l.n == 2)


def test_restated_rule_on_the_shipped_model():
    """The e2w generator at the 25-frame training chunk, by hand from the dispatch's comments: the input conv and the first upsampler take
    32-row chunks, the 3- and 7-tap ResBlocks 128-row chunks, the 11-tap ones 64; every slot pairs."""
    params = dict(in_channels=141, channels=512, kernel_size=7, upsample_scales=[5, 4, 2, 2], upsample_kernel_sizes=[10, 8, 4, 4],
                  resblock_kernel_sizes=[3, 7, 11], resblock_dilations=[[1, 3, 5]] * 3, use_additional_convs=True, bias=True)
    ls = W.generator_wgrad_launches(params, 64, 25)
    assert len(ls) == 4 * 9 + 4 + 1 and not any(l.unpaired for l in ls)
    by = {l.L.name: l for l in ls}
    assert by["input_conv"].kernel == "wgrad_taps_kernel<7,1,32>" and by["upsamples.0.1"].kernel == "wgrad_taps_kernel<2,1,32>"
    assert by["upsamples.1.1"].kernel == "wgrad_taps_kernel<2,1,128>" and by["upsamples.1.1"].rows == 125
    assert by["blocks.0.convs2.0.1"].kernel == "wgrad_taps_kernel<3,1,128>" and by["blocks.1.convs2.2.1"].kernel == "wgrad_taps_kernel<7,1,128>"
    assert by["blocks.2.convs2.2.1"].kernel == "wgrad_taps_kernel<11,1,64>"
    # the last stage is one 32-block wide: its ResBlocks share each chunk's rows between all four waves, its upsampler's phases are 32 wide
    assert {l.L.name.split(".")[1] for l in ls if l.row_split == 4} == {"9", "10", "11"} and by["blocks.11.convs2.0.1"].row_split == 4
    assert [l.L.name for l in ls if l.row_split == 2] == [l.L.name for l in ls if l.g_per_tile == 1] == ["upsamples.3.1"]
