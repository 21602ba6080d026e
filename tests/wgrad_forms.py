"""The weight-gradient dispatch of the generator's backward, restated from articulatory_amd/csrc/hificar_train.hip.inc (line numbers as of
this file's commit), for tests/test_wgrad_forms_host.py and tests/test_gpu_wgrad_forms.py.  Test infrastructure only: no file of the package
imports it, and it imports neither the package nor torch.

``form(layer, rows, n)`` names the instantiation a launch of n = 1 or 2 layers over ``rows`` rows per sequence takes, exactly as the profile
row prints it with HIFICAR_PROFILE_DETAIL=1 ("wgrad_taps_kernel<7,0,128>", "wgrad_gemm_kernel<4,32>", "wgrad_kernel"), with the launch's
row_split and g_per_tile; ``generator_wgrad_launches`` lists every weight-gradient launch of one HiFiGANGenerator backward;
``CASES`` are the GPU cases, chosen from this rule, and ``BUILT`` the instantiations the library builds.  The number of row splits of a launch
(``s..`` in the row) depends on the device's CU count (wgrad_split): it is not predicted here.
"""
import re
from collections import Counter, OrderedDict

MAX_TAPS_ALL = 11  # wgrad_all_taps


def _round_up(x, m):
    return -(-x // m) * m


class Layer:
    """plan_layer (csrc/hificar.hip:316-362): what of a conv layer the weight-gradient rule reads.  cout is per phase for a transposed layer."""

    def __init__(self, name, cin, cin_pad, cout, K, dilation=1, padding=0, transposed=False, stride=1, has_bias=True):
        self.name, self.cin, self.cin_pad, self.cout, self.K, self.has_bias = name, cin, cin_pad, cout, K, has_bias
        assert cin_pad >= 32 and cin_pad % 16 == 0
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
        self.off_min, self.off_max = min(0, min(offs)), max(0, max(offs))
        self.n_blocks32 = cout_pad * self.n_phase // 32
        self.nb32_per_phase = cout_pad // 32

    @property
    def halo(self):
        return self.off_max - self.off_min

    @property
    def n_ablk(self):  # 32-blocks of the A operand; the last one is partial where cin_pad is a multiple of 16 only
        return (self.cin_pad + 31) // 32

    def shape(self):
        """The layer part of the profile row (launch_wgrad_n's kname)."""
        return "%dx%dk%dp%d" % (self.cout, self.cin, self.K, self.n_phase)


def wgrad_all_taps(L):
    """hificar_train.hip.inc:749."""
    return L.ntaps <= MAX_TAPS_ALL


def wgrad_gemm_form(L):
    """hificar_train.hip.inc:753."""
    return L.ntaps == 1 and L.n_phase == 1 and L.n_blocks32 >= 4 and L.n_ablk >= 4


def wgrad_gemm_wide(L):
    """hificar_train.hip.inc:755-757."""
    return L.n_ablk >= 8


def g_per_tile(L):
    """hificar_train.hip.inc:804 / :1018 (wp.g_per_tile): one 32-block per tile where a 64-wide tile would straddle two phases."""
    return 2 if (L.n_phase == 1 or L.nb32_per_phase % 2 == 0) else 1


def wgrad_row_split(L):
    """hificar_train.hip.inc:803-807."""
    nblk = min(g_per_tile(L), L.n_blocks32) * min(2, L.n_ablk)
    return 1 if nblk >= 4 else 2 if nblk >= 2 else 4


def wgrad_chunk_rows(L, rows):
    """hificar_train.hip.inc:764-769."""
    can32 = wgrad_row_split(L) <= 2
    if rows <= 32 and can32:
        return 32
    if L.ntaps <= 7 and rows > 64 and L.halo <= 32:
        return 128
    return 64


def pairs(L0, L1, rows):
    """The pairing rule at the top of launch_wgrad_n (hificar_train.hip.inc:961-968): otherwise a call with two layers runs as two calls of one."""
    return (wgrad_all_taps(L0) and wgrad_all_taps(L1) and L0.ntaps == L1.ntaps and wgrad_chunk_rows(L0, rows) == wgrad_chunk_rows(L1, rows))


def taps_instantiation(ntaps, cr):
    """The NT / EXACT switch of launch_wgrad_n and its HIFICAR_WGT macro (hificar_train.hip.inc:1126-1147)."""
    if ntaps in (1, 2, 3, 7, 11):
        nt, ex = ntaps, 1
    elif ntaps < 7:
        nt, ex = 7, 0
    else:
        nt, ex = 11, 0
    if cr == 128 and nt > 7:
        nt = 7
    return "wgrad_taps_kernel<%d,%d,%d>" % (nt, ex, cr)


def form(L, rows, n=1):
    """(kernel as the detail row names it, row_split, g_per_tile) of a launch of n layers shaped like L (a pair that ``pairs`` admits)."""
    rs, gpt = wgrad_row_split(L), g_per_tile(L)
    if n == 1 and wgrad_gemm_form(L):
        return ("wgrad_gemm_kernel<4,32>" if wgrad_gemm_wide(L) else "wgrad_gemm_kernel<2,64>"), rs, gpt
    if wgrad_all_taps(L):
        return taps_instantiation(L.ntaps, wgrad_chunk_rows(L, rows)), rs, gpt
    return "wgrad_kernel", rs, gpt


# every instantiation the library builds (test_wgrad_forms_host.py checks it against the HIFICAR_WGT switch)
BUILT = frozenset(["wgrad_taps_kernel<%d,1,%d>" % (nt, r) for nt in (1, 2, 3, 7, 11) for r in (32, 64)]
                  + ["wgrad_taps_kernel<%d,0,%d>" % (nt, r) for nt in (7, 11) for r in (32, 64)]
                  + ["wgrad_taps_kernel<%d,1,128>" % nt for nt in (1, 2, 3, 7)] + ["wgrad_taps_kernel<7,0,128>"]
                  + ["wgrad_gemm_kernel<2,64>", "wgrad_gemm_kernel<4,32>", "wgrad_kernel"])


class Launch:
    """One launch_wgrad_n call that reaches a kernel: ``layers`` (1 or 2, the row is named after the first), rows per sequence."""

    def __init__(self, layers, rows, unpaired=False):
        self.layers, self.rows, self.n = layers, rows, len(layers)
        self.unpaired = unpaired  # one half of a two-layer call that ``pairs`` refused
        self.L = layers[0]
        self.kernel, self.row_split, self.g_per_tile = form(self.L, rows, self.n)
        self.chunk = 128 if self.kernel == "wgrad_kernel" else 64 if self.kernel == "wgrad_gemm_kernel<2,64>" else \
            32 if self.kernel == "wgrad_gemm_kernel<4,32>" else wgrad_chunk_rows(self.L, rows)  # kWgR, kWggR, the wide tile's 32 rows
        self.bias = any(l.has_bias for l in layers)

    def row(self):
        """The profile row without its split count."""
        return "%s %s r%d n%d" % (self.kernel, self.L.shape(), self.row_split, self.n)


def generator_wgrad_launches(params, B, T):
    """Every weight-gradient launch of one generator backward (hificar_backward_cond, hificar_train.hip.inc:1429-1513), in its order:
    per stage, last first, each ResBlock slot (conv2 + conv1 as a pair with use_additional_convs, two singles where ``pairs`` refuses), then
    the stage's upsampler on rows / scale; the input conv last."""
    ch, nb = params["channels"], len(params["resblock_kernel_sizes"])
    add, bias = params.get("use_additional_convs", True), params.get("bias", True)
    pad = lambda i: _round_up(ch >> i, 32)  # noqa: E731
    rows_of = [T]
    for s in params["upsample_scales"]:
        rows_of.append(rows_of[-1] * s)
    out = []
    for i in reversed(range(len(params["upsample_scales"]))):
        s, k_up, C, rows = params["upsample_scales"][i], params["upsample_kernel_sizes"][i], ch >> (i + 1), rows_of[i + 1]
        max_d = max(len(d) for d in params["resblock_dilations"])
        for d in reversed(range(max_d)):
            # (block_order / gather_branches: the branches of a dilation step heaviest kernel first; the order does not enter the comparison)
            for j in sorted(range(nb), key=lambda j: -params["resblock_kernel_sizes"][j]):
                if d >= len(params["resblock_dilations"][j]):
                    continue
                k, dil = params["resblock_kernel_sizes"][j], params["resblock_dilations"][j][d]
                base = "blocks.%d" % (i * nb + j)
                c1 = Layer("%s.convs1.%d.1" % (base, d), C, pad(i + 1), C, k, dil, (k - 1) // 2 * dil, has_bias=bias)
                if not add:
                    out.append(Launch([c1], rows))
                    continue
                c2 = Layer("%s.convs2.%d.1" % (base, d), C, pad(i + 1), C, k, 1, (k - 1) // 2, has_bias=bias)
                if pairs(c2, c1, rows):
                    out.append(Launch([c2, c1], rows))
                else:
                    out += [Launch([c2], rows, unpaired=True), Launch([c1], rows, unpaired=True)]
        up = Layer("upsamples.%d.1" % i, ch >> i, pad(i), C, k_up, transposed=True, stride=s, padding=s // 2 + s % 2)
        out.append(Launch([up], rows_of[i]))
    cin = params["in_channels"]
    ks = params["kernel_size"]
    out.append(Launch([Layer("input_conv", cin, max(32, _round_up(cin, 16)), ch, ks, 1, (ks - 1) // 2)], T))
    return out


def expected_rows(launches):
    """{profile row without its split count: launches}."""
    return Counter(l.row() for l in launches)


_SPLIT = re.compile(r" s(\d+) ")


def strip_split(row):
    """("kernel shape rR nN", split count) of a profile row "kernel shape sS rR nN"."""
    m = _SPLIT.search(row)
    assert m, row
    return row[:m.start()] + " " + row[m.end():], int(m.group(1))


# ------------------------------------------------------------------------------------------------ the GPU cases
B = 3


def _params(channels, scales, kernels, dilations, in_channels=141, use_ar=True, kernel_size=7, add=True, bias=True):
    """HiFiGANGenerator keywords of a case: the e2w model's with these sizes; LeakyReLU slope 1 (no kinks but the output conv's and the
    PastFCEncoder's, which the input seed keeps clear of)."""
    assert len(kernels) == len(dilations) <= 4 and in_channels > (128 if use_ar else 0)
    return dict(in_channels=in_channels, out_channels=1, channels=channels, kernel_size=kernel_size, upsample_scales=list(scales),
                upsample_kernel_sizes=[2 * s for s in scales], resblock_kernel_sizes=list(kernels), resblock_dilations=[list(d) for d in dilations],
                use_additional_convs=add, bias=bias, nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 1.0},
                use_weight_norm=True, use_ar=use_ar, ar_input=512, ar_hidden=256, ar_output=128)


# name -> (params, T).  Stage widths, kernels and T follow the table of conditions in test_wgrad_forms_host.py, which proves the choice.
CASES = OrderedDict([
    # 24 rows per sequence in the stage (R = 32, one partly filled chunk): NT 1, 3, 7 exact and 7 inexact; the upsampler's two taps at R = 32
    # over 8 rows; the input conv's 144-float pitch (a partial 32-block of A) at R = 32; width 48: an output width no multiple of 32
    ("r32_k1357", (_params(96, [3], [1, 3, 5, 7], [[1], [1, 2], [1], [1, 3]]), 8)),
    # ... NT 11 exact and inexact at R = 32; kernel 11 at dilation 5: a halo of 50 rows over 32-row chunks; ResBlocks without bias
    ("r32_k911", (_params(96, [3], [9, 11], [[1, 2], [1, 5]], bias=False), 8)),
    # 48 rows (R = 64, partly filled): every taps form at R = 64, the upsampler over 16 rows at scale 3
    ("r64_k1357", (_params(96, [3], [1, 3, 5, 7], [[1], [1], [2], [1]]), 16)),
    # 150 rows: kernels 9 and 11 keep 64-row chunks (three per sequence, the last partly filled); the upsampler's two taps at R = 64 (50 rows)
    ("r64_k911_150", (_params(200, [3], [9, 11], [[1], [1, 5]], in_channels=150), 50)),
    # 150 rows in the second stage: R = 128 for NT 1, 3, 7 exact and 7 inexact (two chunks per sequence), the second upsampler's two taps at
    # R = 128 over 75 rows; kernel 7 at dilation 6 (halo 36) takes R = 64 where its conv2 takes 128: a pair that runs as two singles
    ("r128_k1357", (_params(192, [3, 2], [1, 3, 5, 7], [[1], [1, 3], [1, 2], [1, 6]]), 25)),
    # the same slots one conv each (use_additional_convs = False): single launches of the shapes the case above pairs
    ("r128_single", (_params(192, [3, 2], [1, 3, 5, 7], [[1], [1, 3], [1, 2], [1, 6]], add=False), 25)),
    # kernels 13 and 15: the per-tap kernel over 150 rows (two 128-row chunks per sequence, the second partly filled) at width 48
    # (row_split 1); pairs that fall back to two singles
    ("pertap_w48", (_params(96, [3], [13, 15], [[1, 2], [1]]), 50)),
    # ... at width 24 (row_split 4) over 32 rows, after a scale-4 upsampler into one 32-block per phase (g_per_tile 1 at an even scale,
    # row_split 2); the taps kernel at row_split 4: R = 64 although the stage has 32 rows (can32 false)
    ("pertap_w24", (_params(48, [4], [13, 3, 7], [[1], [1, 2], [3]]), 8)),
    # ... at width 16 over 150 rows (row_split 4, two chunks); the input conv with kernel 13 from 40 channels (pitch 48: a partial
    # 32-block of A) into 32: the per-tap kernel at row_split 2; without the AR branch
    ("pertap_in32", (_params(32, [3], [13], [[1]], in_channels=40, use_ar=False, kernel_size=13), 50)),
    # width 24 over 150 rows: the taps kernel at row_split 4 with R = 128 (kernel 3) and R = 64 (kernel 9), two and three chunks per
    # sequence; g_per_tile 1 at an odd scale (row_split 2, R = 64 over 50 rows); ResBlocks without bias
    ("w24_150", (_params(48, [3], [3, 9], [[1, 3], [2]], bias=False), 50)),
    # the one-tap GEMM forms: the input conv with kernel 1 from 141 channels (pitch 144: a partial A tile) into 256: <2,64>; kernel-1
    # ResBlocks at width 128 paired: the taps kernel, its split count from the GEMM branch of wgrad_split
    ("gemm_pair", (_params(256, [2], [1], [[1, 1]], kernel_size=1), 40)),
    # ... and one conv per slot: <2,64> at width 128; the input conv from 241 channels: <4,32>
    ("gemm_single", (_params(256, [2], [1], [[1]], in_channels=241, kernel_size=1, add=False), 40)),
    # width 256, one conv per slot: <4,32> beside a 3-tap layer of the same width; the input conv from 200 channels (pitch 208, seven
    # 32-blocks of A, the last one half) into 512: <2,64> with a partial tile in both directions of A
    ("gemm_wide", (_params(512, [2], [1, 3], [[1], [1]], in_channels=200, kernel_size=1, add=False), 33)),
])


def case_launches(name):
    params, T = CASES[name]
    return generator_wgrad_launches(params, B, T)
