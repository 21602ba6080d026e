"""The discriminators' per-layer, per-call choice of form, restated from articulatory_amd/csrc/hificar_disc.hip.inc (disc_add_layer, disc_geom,
disc_plan, the launchers of hificar_disc_forward / hificar_disc_backward) and hificar_disc_kernels.hip.h, for tests/test_disc_forms_host.py
and tests/test_gpu_disc_forms.py.  Test infrastructure only: no file of the package imports it, and it imports neither the package nor torch.

A conv layer of a sub-discriminator runs, in one call over (B, T), as
  * the im2col form: a gather into A [M][Kg_pad] (M = every output row of every sequence), one GEMM per group, the data gradient the same GEMM
    on the transposed pack followed by a tap sum (col2im), the weight gradient a one-tap launch over A; or
  * the window form (polyphase input): a gather into the zero-padded activations X [seq][Lp][cin_g], Lp = stride * (L_out + ntaps - 1), read as
    rows of ``stride`` positions by a ceil(k / stride)-tap stride-1 conv; the data gradient a conv that writes dX at the padded positions
    (col2im reads ONE row, t + pad, where that row exists), the weight gradient the all-taps kernel over X's rows with a remap
    (tap q, r * cin_g + c) -> kernel index stride * q + r (slots >= k dropped).
``plan(params, B, T)`` lists, per layer of every sub-discriminator, which form the call takes and which of the scalar / 4-wide gathers, and
``expected_rows`` the profile rows one forward + backward then produces under HIFICAR_PROFILE_DETAIL=1.  ``CASES`` are the GPU cases, chosen
from this rule; the host test proves what they reach.  The weight-gradient instantiation and its split count are not predicted here
(tests/wgrad_forms.py does that for the generator): only the layer-shape part of the row.
"""
from collections import Counter, OrderedDict

WINDOW_MIN_ROWS = 32  # hificar_disc::window_min_rows
MAX_WINDOW_TAPS = 11  # disc_add_layer: ntaps_p <= 11 (the all-taps weight-gradient kernel's limit)


def _round_up(x, m):
    return -(-x // m) * m


def disc_out_len(L, k, stride, pad):
    """disc_out_len: an input shorter than the kernel has no output position."""
    return 0 if L + 2 * pad < k else (L + 2 * pad - k) // stride + 1


class Layer:
    """disc_add_layer: what of a conv layer the rule reads.  ``first``: layer 0 of its stack (reads the signal, never a window)."""

    def __init__(self, base, cin, cout, k, stride, pad, groups, act=True, bias=True, conv2d=False, first=False):
        assert cin % groups == 0 and cout % groups == 0
        self.base, self.cin, self.cout, self.k, self.stride, self.pad, self.groups = base, cin, cout, k, stride, pad, groups
        self.act, self.bias, self.conv2d, self.first = act, bias, conv2d, first
        self.cin_g, self.cout_g = cin // groups, cout // groups
        self.Kg = self.cin_g * k
        self.Kg_pad, self.Np = _round_up(self.Kg, 32), _round_up(self.cout_g, 32)
        self.ntaps = -(-k // stride)  # taps of the polyphase-input conv
        self.can_window = (not conv2d and not first and k > 1 and self.cin_g % 4 == 0 and (stride * self.cin_g) % 32 == 0
                           and 2 <= self.ntaps <= MAX_WINDOW_TAPS)

    def dropped_slots(self):
        """Kernel indices stride * q + r of the polyphase pack (modes 10 / 11, the weight gradient's poly remap) that carry no weight."""
        return [self.stride * q + r for q in range(self.ntaps) for r in range(self.stride) if self.stride * q + r >= self.k]


def scale_layers(prefix, in_channels=1, out_channels=1, kernel_sizes=(15, 41, 5, 3), channels=128, max_downsample_channels=1024, max_groups=16,
                 bias=True, downsample_scales=(2, 2, 4, 4, 1), **_ignored):
    """The Conv1d stack of one scale discriminator (articulatory_amd.utils.synth.scale_disc_layers; the host test compares the two)."""
    spec = [(in_channels, channels, kernel_sizes[0], 1, 1)]
    in_chs, out_chs, groups = channels, channels, 4
    for s in downsample_scales:
        spec.append((in_chs, out_chs, kernel_sizes[1], s, groups))
        in_chs = out_chs
        out_chs = min(in_chs * 2, max_downsample_channels)
        groups = min(groups * 4, max_groups)
    out_chs = min(in_chs * 2, max_downsample_channels)
    spec.append((in_chs, out_chs, kernel_sizes[2], 1, 1))
    spec.append((out_chs, out_channels, kernel_sizes[3], 1, 1))
    n = len(spec)
    return [Layer("%s.layers.%d%s" % (prefix, l, ".0" if l + 1 < n else ""), cin, cout, k, s, (k - 1) // 2, g, act=l + 1 < n, bias=bias, first=l == 0)
            for l, (cin, cout, k, s, g) in enumerate(spec)]


def period_layers(prefix, in_channels=1, out_channels=1, kernel_sizes=(5, 3), channels=32, downsample_scales=(3, 3, 3, 3, 1),
                  max_downsample_channels=1024, **_ignored):
    """The Conv2d (k, 1) stack of one period discriminator (period_disc_layers): the output conv has kernel_sizes[1] - 1 taps."""
    out = []
    in_chs, out_chs = in_channels, channels
    for l, s in enumerate(downsample_scales):
        out.append(Layer("%s.convs.%d.0" % (prefix, l), in_chs, out_chs, kernel_sizes[0], s, (kernel_sizes[0] - 1) // 2, 1, conv2d=True, first=l == 0))
        in_chs = out_chs
        out_chs = min(out_chs * 4, max_downsample_channels)
    out.append(Layer(prefix + ".output_conv", out_chs, out_channels, kernel_sizes[1] - 1, 1, (kernel_sizes[1] - 1) // 2, 1, act=False, conv2d=True))
    return out


def layers_from_dicts(prefix, dicts):
    """A scale discriminator's stack from the dicts articulatory_amd.utils.synth.scale_disc_layers returns (cin, cout, k, stride, groups, act, bias, pad)."""
    return [Layer("%s.layers.%d%s" % (prefix, l, ".0" if d["act"] else ""), d["cin"], d["cout"], d["k"], d["stride"], d["pad"], d["groups"], act=d["act"],
                  bias=d["bias"], first=l == 0) for l, d in enumerate(dicts)]


class Sub:
    def __init__(self, layers, period=0, scale=0):
        self.layers, self.period, self.scale = layers, period, scale


def subs_of(params, scale_dicts=None):
    """hificar_disc_create's order: the scale discriminators, then the period discriminators.  ``params``: the full dict (every key of the
    multi-scale multi-period class).  ``scale_dicts``: the scale discriminators' layers as dicts instead of scale_discriminator_params."""
    mk = (lambda prefix: layers_from_dicts(prefix, scale_dicts)) if scale_dicts else (lambda prefix: scale_layers(prefix, **params["scale_discriminator_params"]))
    out = [Sub(mk("msd.discriminators.%d" % i), scale=i) for i in range(params["scales"])]
    out += [Sub(period_layers("mpd.discriminators.%d" % i, **params["period_discriminator_params"]), period=p) for i, p in enumerate(params["periods"])]
    return out


def disc_geom(sub, pool, B, T):
    """disc_geom: (sequences, rows per sequence of the input and of every layer's output)."""
    if sub.period == 0:
        t = T
        for _ in range(sub.scale):
            t = disc_out_len(t, pool["kernel_size"], pool["stride"], pool["padding"])
        nseq, L = B, [t]
    else:
        nseq, L = B * sub.period, [-(-T // sub.period)]
    for layer in sub.layers:
        L.append(disc_out_len(L[-1], layer.k, layer.stride, layer.pad))
    return nseq, L


def window_geometry(k, stride, pad, L_in):
    """(L_out, ntaps, Lp) of the window form."""
    L_out, ntaps = disc_out_len(L_in, k, stride, pad), -(-k // stride)
    return L_out, ntaps, stride * (L_out + ntaps - 1)


def window_invariants(k, stride, pad, L_in, guarded=True):
    """The three geometry invariants of the window form, each True where it holds:
      forward  every padded position the forward reads (t_out * stride + tap) is a row of X: < Lp
      col2im   every row the col2im reads is a row of dX: t + pad < Lp for every t < L_in it reads.  ``guarded``: the kernels read the row
               only where t + pad < Lp (a position past the window is read by no output: its gradient is zero); False: the read as it was
               before that guard, every t < L_in
      dropped  every polyphase slot stride * q + r without a weight has index >= k, i.e. no slot below k is lost: stride * ntaps >= k"""
    L_out, ntaps, Lp = window_geometry(k, stride, pad, L_in)
    forward = stride * (L_out - 1) + k - 1 < Lp
    rows_read = range(pad, min(L_in + pad, Lp) if guarded else L_in + pad)  # t + pad for the t < L_in whose window row is fetched
    slots = range(stride * ntaps)  # stride * q + r; the pack and the weight-gradient remap keep those below k
    dropped = len([s for s in slots if s < k]) == k and all(s >= k for s in slots[k:])
    return forward, rows_read[-1] < Lp, dropped


class Run:
    """One layer in one call: the decisions of disc_plan and of the two gather launchers."""

    def __init__(self, sub, l, nseq, L_in, L_out, vec4_enabled=True):
        layer, prev = sub.layers[l], (sub.layers[l - 1] if l else None)
        nxt = sub.layers[l + 1] if l + 1 < len(sub.layers) else None
        self.sub, self.l, self.layer, self.prev, self.next = sub, l, layer, prev, nxt
        self.nseq, self.L_in, self.rows, self.M = nseq, L_in, L_out, nseq * L_out
        # disc_plan: use_windows && can_window && prev.cout_g % 4 == 0 && L_out >= window_min_rows
        self.window = bool(layer.can_window and prev.cout_g % 4 == 0 and L_out >= WINDOW_MIN_ROWS)
        self.denied_by_prev = bool(layer.can_window and prev.cout_g % 4 != 0 and L_out >= WINDOW_MIN_ROWS)
        self.Lp = layer.stride * (L_out + layer.ntaps - 1) if self.window else 0
        # input positions at the end that no output reads
        self.tail = (L_in + 2 * layer.pad - layer.k) % layer.stride if L_out > 0 else 0
        # hificar_disc_forward: im2col4_kernel for a previous-layer gather with 4 | cin_g and 4 | prev.cout_g (pitches, strides and bases are
        # multiples of 4 floats / 16 bytes by construction: Np and Kg_pad are multiples of 32, the buffers' offsets of 1024 bytes)
        self.fwd_vec4 = bool(vec4_enabled and prev is not None and layer.cin_g % 4 == 0 and prev.cout_g % 4 == 0)
        # hificar_disc_backward, dZ of THIS layer from the next layer's dA: col2im_mask4_kernel with 4 | cout_g and 4 | next.cin_g (and the loss's
        # gradient buffers on 16-byte boundaries: torch's allocations are)
        self.col2im_vec4 = None if nxt is None else bool(vec4_enabled and layer.cout_g % 4 == 0 and nxt.cin_g % 4 == 0)

    def reads(self):
        """What the three passes of this layer read: {"forward": ..., "dgrad": ..., "wgrad": ...}, each (what, rows per sequence, floats per row)."""
        L = self.layer
        if self.window:
            return {"forward": ("X rows of %d padded positions, %d taps" % (L.stride, L.ntaps), self.Lp // L.stride, L.stride * L.cin_g),
                    "dgrad": ("dZ rows, %d taps, padding %d; writes dX at padded positions" % (L.ntaps, L.ntaps - 1), self.rows, L.Np),
                    "wgrad": ("X rows, all taps; (q, r * cin_g + c) -> k index %d q + r, %d slots dropped" % (L.stride, len(L.dropped_slots())),
                              self.Lp // L.stride, L.stride * L.cin_g)}
        return {"forward": ("im2col matrix A", self.rows, L.Kg_pad), "dgrad": ("dZ rows; writes dA", self.rows, L.Np),
                "wgrad": ("A rows, one tap; a = tap * cin_g + c", self.rows, L.Kg_pad)}

    # ---- profile rows
    def conv_rows(self, dx=True):
        out = [self.layer.base + ("#g0#poly x1" if self.window else "#g0 x1")]
        if self.window:
            out.append(self.layer.base + "#g0#polydgrad x1")
        elif self.l > 0 or dx:
            out.append(self.layer.base + "#g0#dgrad x1")
        return out

    def gather_rows(self):
        out = ["im2col_kernel|%s v%d" % (self.layer.base, 4 if self.fwd_vec4 else 1)]
        if self.next is not None:
            out.append("col2im_mask_kernel|%s v%d" % (self.layer.base, 4 if self.col2im_vec4 else 1))
        return out

    def wgrad_shape(self):
        """The layer part of the weight-gradient row (launch_wgrad_n's kname: cout x cin k K p n_phase of the ConvLayer it runs on)."""
        L = self.layer
        return "%dx%dk%dp1" % ((L.cout_g, L.stride * L.cin_g, L.ntaps) if self.window else (L.cout_g, L.Kg, 1))


def plan(params, B, T, vec4_enabled=True, scale_dicts=None):
    """Every layer of every sub-discriminator in one call, in hificar_disc_create's order."""
    out = []
    for sub in subs_of(params, scale_dicts):
        nseq, L = disc_geom(sub, params["scale_downsample_pooling_params"], B, T)
        out += [Run(sub, l, nseq, L[l], L[l + 1], vec4_enabled) for l in range(len(sub.layers))]
    return out


def admits(params, B, T):
    """hificar_disc_forward's argument checks: reflect padding needs T > the pad; every layer at least one row."""
    if T < 2 or any((p - T % p) % p >= T for p in params["periods"]):
        return False
    return all(r.M >= 1 for r in plan(params, B, T))


def expected_rows(params, B, T, vec4_enabled=True, scale_dicts=None):
    """(conv rows, gather rows, weight-gradient shapes, (weight reductions, bias reductions)) of one forward + backward of every layer output
    with respect to every parameter and x.  Counters: a row is one launch per layer."""
    runs = plan(params, B, T, vec4_enabled, scale_dicts)
    conv = Counter(r for run in runs for r in run.conv_rows())
    gather = Counter(r for run in runs for r in run.gather_rows())
    wgrad = Counter(run.wgrad_shape() for run in runs)
    return conv, gather, wgrad, (len(runs), sum(run.layer.bias for run in runs))


# ------------------------------------------------------------------------------------------------ the GPU cases
POOL_422 = {"kernel_size": 4, "stride": 2, "padding": 2}
POOL_321 = {"kernel_size": 3, "stride": 2, "padding": 1}
PERIODS = [2, 3, 5, 7, 11]


def _scale(channels, max_channels, max_groups, kernels, scales, slope=1.0):
    return {"in_channels": 1, "out_channels": 1, "kernel_sizes": list(kernels), "channels": channels, "max_downsample_channels": max_channels,
            "max_groups": max_groups, "bias": True, "downsample_scales": list(scales), "nonlinear_activation": "LeakyReLU",
            "nonlinear_activation_params": {"negative_slope": slope}}


def _period(channels, max_channels, scales, slope=1.0):
    return {"in_channels": 1, "out_channels": 1, "kernel_sizes": [5, 3], "channels": channels, "downsample_scales": list(scales),
            "max_downsample_channels": max_channels, "bias": True, "nonlinear_activation": "LeakyReLU",
            "nonlinear_activation_params": {"negative_slope": slope}, "use_weight_norm": True, "use_spectral_norm": False}


def _msd(scales, pool, sp):
    return dict(scales=scales, scale_downsample_pooling="AvgPool1d", scale_downsample_pooling_params=dict(pool), scale_discriminator_params=sp,
                follow_official_norm=True, periods=[], period_discriminator_params=_period(4, 16, [3, 1]))


def _mpd(pp):
    return dict(scales=0, scale_downsample_pooling="AvgPool1d", scale_downsample_pooling_params=dict(POOL_422),
                scale_discriminator_params=_scale(16, 64, 4, [15, 41, 5, 3], [4, 4, 1]), follow_official_norm=True, periods=list(PERIODS),
                period_discriminator_params=pp)


# LeakyReLU slope 1 (the identity: no kinks; every form, gather and reduction still runs) unless a case says otherwise
CONFIG_A = _scale(32, 128, 4, [15, 41, 5, 3], [4, 4, 1])     # strided layers 41 taps at stride 4: 11 polyphase taps, 3 of 44 slots dropped
CONFIG_B = _scale(32, 128, 16, [5, 11, 5, 3], [2, 2, 1])     # stride * cin_g = 16, 4, 4: the grouped layers never take the window; groups 4, 16, 16
CONFIG_C = _scale(64, 128, 4, [5, 3, 5, 3], [2, 2, 1])       # 3 taps at stride 2: 2 polyphase taps, 1 of 4 slots dropped
CONFIG_D = _scale(64, 128, 4, [15, 41, 5, 3], [2, 2])        # 41 taps at stride 2: 21 polyphase taps, more than the window form has
CONFIG_E = _scale(128, 128, 16, [15, 41, 5, 3], [4, 4, 1])   # the second strided layer: 16 groups of 8 channels, window-capable at stride 4
CONFIG_F = _scale(48, 96, 16, [5, 11, 5, 3], [2, 2])         # 16 groups of 3 -> 6 channels: scalar gathers; the next layer is refused its window
PERIOD_6 = _period(6, 24, [3, 1])                            # 6 channels: no multiple of 4
PERIOD_8 = _period(8, 32, [3, 3, 1])

# name -> (params, B, T).  tests/test_disc_forms_host.py proves from the rule what each comment claims.
CASES = OrderedDict([
    # scale 0: layer 1 at 128 rows (window), layer 2 at exactly 32 rows (window; 3 of its 128 input rows unread), layers 4 and 5 at 32 rows
    # (window, stride 1, 5 and 3 taps); scale 1 (255 samples): the same shapes at 64 rows (window) and 16 rows (im2col, 3 input rows unread)
    ("a_509", (_msd(2, POOL_422, CONFIG_A), 2, 509)),
    # scale 0: layer 1 at 121 rows (window, 3 of 484 input rows unread), layer 2 at 31 rows: im2col, as layers 4 and 5
    ("a_484", (_msd(2, POOL_422, CONFIG_A), 2, 484)),
    # stride-1 layers at 32 rows (window) and, after an AvgPool1d(3, 2, 1) to 64 samples, at 16 rows (im2col); 16 groups
    ("b_127", (_msd(2, POOL_321, CONFIG_B), 3, 127)),
    # ... at 33 and 17 rows, the pooled signal 65 samples
    ("b_130", (_msd(2, POOL_321, CONFIG_B), 3, 130)),
    # window layers at stride 2 with two taps, 70 and 35 rows, each with one unread input row
    ("c_140", (_msd(1, POOL_422, CONFIG_C), 3, 140)),
    # 21 polyphase taps at 75 and 38 rows: im2col
    ("d_150", (_msd(1, POOL_422, CONFIG_D), 2, 150)),
    # 16 groups in the window form at exactly 32 rows, 3 input rows unread
    ("e_512", (_msd(1, POOL_422, CONFIG_E), 2, 512)),
    # scalar gathers (cin_g 3, previous cout_g 6); layer 3 (96 channels, one group, 38 rows) refused its window by layer 2's 6 channels per group
    ("f_150", (_msd(1, POOL_422, CONFIG_F), 2, 150)),
    # periods: T a multiple of every period (no reflect padding), 6 channels
    ("p6_2310", (_mpd(PERIOD_6), 2, 2310)),
    # ... T = 1 modulo every period: the maximal reflect padding, period - 1
    ("p8_2311", (_mpd(PERIOD_8), 2, 2311)),
    # the smallest T the stacks admit: period 11 pads 5 of 6 samples, periods 7 and 11 run every layer on one row per column
    ("p8_6", (_mpd(PERIOD_8), 3, 6)),
    # ... and one above it (period 11 pads 4 of 7), 6 channels
    ("p6_7", (_mpd(PERIOD_6), 3, 7)),
])

# the one kinked run per form: config A at T = 509 with LeakyReLU(0.1) (the input seed keeps every pre-activation clear of zero)
KINKED = ("a_509_kink", (_msd(2, POOL_422, _scale(32, 128, 4, [15, 41, 5, 3], [4, 4, 1], slope=0.1)), 2, 509))

# a geometry the Python classes never build (an even kernel without padding) but hificar_disc_create accepts: layer 1 as k = 4, stride 2, pad 0
# on 16 channels per group.  T = 69: L_in = 69, L_out = 33, two polyphase taps, Lp = 68 < L_in + pad = 69: row 68 of dX does not exist.
ODD_LAYERS = [dict(cin=1, cout=32, k=5, stride=1, groups=1, act=True, bias=True, pad=2),
              dict(cin=32, cout=32, k=4, stride=2, groups=2, act=True, bias=True, pad=0),
              dict(cin=32, cout=1, k=3, stride=1, groups=1, act=False, bias=True, pad=1)]
ODD_B, ODD_T = 3, 69
ODD_PARAMS = _msd(1, POOL_422, _scale(32, 32, 2, [5, 3, 3, 3], [2]))  # (the sub-dict is not read: ODD_LAYERS replaces the stack it describes)


def case_runs(name, vec4_enabled=True):
    params, B, T = CASES[name] if name in CASES else KINKED[1]
    return plan(params, B, T, vec4_enabled)
