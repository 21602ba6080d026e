"""What the Transformer's bf16x3wac training arithmetic adds to bf16x3wa's launches, restated in Python from the library's rule, and the layout of
its tap-column split pass restated in numpy.  Shared by tests/test_transformer_train_bf16x3wac_host.py and
tests/test_gpu_transformer_train_bf16x3wac.py (which holds the device's profile rows to it).  Test infrastructure only.

The rule (csrc/hificar_xfmr_train.hip.inc: wgrad_gemm3_form, XfmrTrainCtx::wgrad): the weight gradient of a conv with three taps, one phase,
at least four 32-blocks of output channels and of input columns, and 3 cin_pad <= 3072 runs as the one-tap GEMM G^T A3 of a (cout, 3 cin_pad)
layer in wgrad_bf16x3_kernel<4,32> (3 cin_pad >= 384 columns are at least 12 column blocks: always the 128 x 256 tile), over the step's rows as
one run — B T (dense, ragged) or the packed rows — with the split count wgrad_split gives that one-tap layer.  Its profile row carries the conv's
own shape (cout x cin k3 p1).  One G split (xfmr_split_rows_t_kernel) and one tap-column split (xfmr_split_taps_t_kernel) per such launch.
Every one-tap GEMM-form layer is bf16x3w's (tests/transformer_bf16x3w_forms.py); what is left runs in the fp32 kernels.

The tap-column layout: fp32 rows [M][C] -> [ceil(M / 8)][3 C][hi 8 | lo 8] bf16, column k C + c of row r = row r + k - 1 of channel c, zero
bits where that row is outside [0, M), not a frame (a padded frame, a gap row) or in another sequence than row r.
"""

import numpy as np

import transformer_bf16x3w_forms as W
import transformer_train_oracle as O

FF = W.FF
# One case more than the oracle modules' shapes offer: in_channels = 101 pads to 128 columns, so conv_blocks.0.conv1 moves with cin_pad != cin —
# the taps lie 128 columns apart in the partial and 101 apart in the gradient (wreduce's gemm_pitch), and the gradient's rows start on no
# 16-byte boundary.  In O.SHAPES' layout; drawn through O.case(name, shapes=EXTRA_SHAPES) under a seed registered here.
EXTRA_SHAPES = {"pad101": (dict(in_channels=101, out_channels=8, elayers=1, hidden_dim=128), 2, 65, 0.2)}
O.SEEDS.setdefault("pad101", 8701)
DENSE_CASES = ("t2", "t65", "nores", "d48", "rows1380", "rows4112", "pad101")
RAGGED_CASES = ("mixed", "nores")                        # of transformer_ragged_oracle.RAGGED_SHAPES, each padded ("ragged") and packed


def case_shapes(name):
    """The ``shapes`` argument of O.case / O.restatement for a dense case."""
    return EXTRA_SHAPES if name in EXTRA_SHAPES else O.EDGE_SHAPES if name in O.EDGE_SHAPES else None


def case_shape(name):
    """(params, B, T) of a GPU case."""
    return EXTRA_SHAPES[name][:3] if name in EXTRA_SHAPES else W.case_shape(name)


def case_rows(name, form="dense"):
    if name in EXTRA_SHAPES:
        return EXTRA_SHAPES[name][1] * EXTRA_SHAPES[name][2]
    return W.case_rows(name, form)


def pad32(n):
    return W.blocks32(n) * 32


def gemm3_form(L):
    return L.K == 3 and W.blocks32(L.cout) >= 4 and W.blocks32(L.cin) >= 4 and 3 * pad32(L.cin) <= FF


def twin(L):
    """The one-tap layer whose weight gradient is the conv's: (cout, 3 cin_pad)."""
    return W.Layer(L.name, L.cout, 3 * pad32(L.cin), 1, L.bias)


def launch(L, rows, num_cus=W.NUM_CUS):
    """The wgrad_bf16x3_kernel launch of a selected conv: W.launch of its twin, under the conv's own Layer."""
    t = W.launch(twin(L), rows, num_cus)
    assert (t.aj, t.rchunk) == (4, 32)
    return t._replace(layer=L)


def case_launches(name, form="dense", num_cus=W.NUM_CUS):
    """(the k = 3 launches bf16x3wac moves to wgrad_bf16x3_kernel, bf16x3w's one-tap launches, the layers that stay on the fp32 kernels)."""
    params = case_shape(name)[0]
    rows = case_rows(name, form)
    ls = W.layers(params)
    return ([launch(L, rows, num_cus) for L in ls if gemm3_form(L)], [W.launch(L, rows, num_cus) for L in ls if W.gemm_form(L)],
            [L for L in ls if not gemm3_form(L) and not W.gemm_form(L)])


def row_key(l):
    """The profile row of a moved launch under HIFICAR_PROFILE_DETAIL=1 without its split count: the conv's own shape."""
    return f"wgrad_bf16x3_kernel<{l.aj},{l.rchunk}> {l.layer.cout}x{l.layer.cin}k3p1", "r1 n1"


def expected_rows(launches):
    """{(row without its split count): (launches, split count)} of the moved launches."""
    out = {}
    for l in launches:
        k = row_key(l)
        n, s = out.get(k, (0, l.nsplit))
        assert s == l.nsplit
        out[k] = (n + 1, s)
    return out


def moved_tensors(params):
    """The state_dict names whose gradients bf16x3wac computes on bf16 MFMAs and bf16x3wa does not."""
    return [f"{L.name}.{t}" for L in W.layers(params) if gemm3_form(L) for t in ("weight", "bias")]


# ------------------------------------------------------------------------------------------------ the tap-column split pass
def tap_columns(x, T=0, valid=None, packed=False):
    """fp32 rows x [M][C] -> A3 [M][3 C] (float32): column k C + c of row r is x[r + k - 1, c], and +0 where row r + k - 1 is outside
    [0, M), not ``valid`` (bool [M]; whatever x holds there) or — dense and ragged: sequences of T rows (T = 0: one of M rows) — in another
    sequence than row r.  packed: one run of rows, the gap rows (not valid) are the sequences' ends."""
    M, C = x.shape
    keep = np.ones(M, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    seq = np.zeros(M, dtype=np.int64) if packed or T == 0 else np.arange(M) // T
    out = np.zeros((M, 3 * C), dtype=np.float32)
    for k in range(3):
        for r in range(M):
            s = r + k - 1
            if 0 <= s < M and keep[s] and seq[s] == seq[r]:
                out[r, k * C:(k + 1) * C] = x[s]
    return out


def split_taps_t(x, T=0, valid=None, packed=False):
    """The bytes of [ceil(M / 8)][3 C][hi 8 | lo 8] bf16 of tap_columns(x, ...): rows past M are zero bits."""
    return W.split_rows_t(tap_columns(x, T, valid, packed))
