"""What the Transformer's bf16x3w training arithmetic launches, restated in Python from the library's rule, and the layout of its split pass
restated in numpy.  Shared by tests/test_transformer_train_bf16x3w_host.py (which proves from the rule that the GPU cases reach every path of
wgrad_bf16x3_kernel) and tests/test_gpu_transformer_train_bf16x3w.py (which holds the device's profile rows to it).  Test infrastructure only.

The rule (csrc/hificar_train.hip.inc: wgrad_gemm_form, wgrad_gemm_wide, wgrad_split; csrc/hificar_xfmr_train.hip.inc: XfmrTrainCtx::wgrad):
a layer's weight gradient runs in wgrad_bf16x3_kernel when the layer has one tap and at least four 32-blocks of output channels and of input
columns; <4,32> (a 128 x 256 tile on 32-row chunks) when it has at least eight 32-blocks of input columns, else <2,64> (128 x 128 on 64-row
chunks).  The rows are the step's: B T (dense, ragged) or the packed rows.  The split count is the fp32 form's.
"""

from collections import namedtuple

import numpy as np

import transformer_ragged_oracle as R
import transformer_train_oracle as O

NUM_CUS = 256  # MI355X; the split count depends on it (the GPU test reads the device's and compares)
FF = 3072
# of O.SHAPES / O.EDGE_SHAPES.  rows1380: the one case in which a split of the 128 x 128 tile owns three chunks (its two-buffer ring wraps):
# linear1 at 128 columns, 22 chunks over 10 splits; the wide tile has rows4112 for that.
DENSE_CASES = ("t2", "t65", "d48", "rows4112", "nores", "rows1380")
RAGGED_CASE = "mixed"                                    # of R.RAGGED_SHAPES, padded ("ragged") and packed
PACK_GRANULE = 256

Layer = namedtuple("Layer", "name cout cin K bias")
Launch = namedtuple("Launch", "layer aj rchunk rows tiles_g tiles_a nsplit nchunks")


def case_shape(name):
    """(params, B, T) of a GPU case."""
    if name in O.SHAPES:
        return O.SHAPES[name][:3]
    if name in O.EDGE_SHAPES:
        return O.EDGE_SHAPES[name][:3]
    return R.RAGGED_SHAPES[name][:3]


def case_rows(name, form="dense"):
    """The GEMM rows of a case's step: B T, or for the packed form of the ragged case sum (length + 1) rounded up to 256."""
    params, B, T = case_shape(name)
    if form != "packed":
        return B * T
    lengths = R.RAGGED_SHAPES[name][3]
    return (sum(lengths) + B + PACK_GRANULE - 1) // PACK_GRANULE * PACK_GRANULE


def layers(params):
    """Every layer with a weight gradient, in the order of the backward pass: (name, cout, cin, K, has a bias)."""
    F, C, out, E = params["hidden_dim"], params["in_channels"], params["out_channels"], params["elayers"]
    ls = [Layer("w_out", out, F, 1, True)]
    for l in reversed(range(E)):
        ls += [Layer(f"layers.{l}.linear2", F, FF, 1, True), Layer(f"layers.{l}.linear1", FF, F, 1, True), Layer(f"layers.{l}.w_o", F, F, 1, False),
               Layer(f"layers.{l}.qkv", 3 * F, F, 1, False)]
    ls.append(Layer("w_raw_in", F, F, 1, True))
    for i in reversed(range(3)):
        cin = C if i == 0 else F
        ls += [Layer(f"conv_blocks.{i}.conv2", F, F, 3, True), Layer(f"conv_blocks.{i}.conv1", F, cin, 3, True)]
        if i == 0 and C != F:
            ls.append(Layer("conv_blocks.0.residual_path", F, C, 1, True))
    return ls


def blocks32(n):
    return (n + 31) // 32


def gemm_form(L):
    return L.K == 1 and blocks32(L.cout) >= 4 and blocks32(L.cin) >= 4


def gemm_wide(L):
    return blocks32(L.cin) >= 8


def wgrad_split(L, rows, num_cus=NUM_CUS):
    """wgrad_split of a GEMM-form layer over one sequence of `rows` rows."""
    aw = 8 if gemm_wide(L) else 4
    tiles = ((blocks32(L.cout) + 3) // 4) * ((blocks32(L.cin) + aw - 1) // aw)
    nchunks = (rows + 63) // 64
    if tiles * 16 <= num_cus:
        return max(1, min(num_cus // tiles, 256, nchunks))
    best, best_cost = 1, 1e300
    for sp in range(1, min(16, nchunks) + 1):
        cost = ((tiles * sp + num_cus - 1) // num_cus) / sp * (1.0 + 0.02 * (sp - 1))
        if cost < best_cost - 1e-9:
            best, best_cost = sp, cost
    return best


def launch(L, rows, num_cus=NUM_CUS):
    aj, rchunk = (4, 32) if gemm_wide(L) else (2, 64)
    groups = (rows + 7) // 8
    return Launch(L, aj, rchunk, rows, (blocks32(L.cout) + 3) // 4, (blocks32(L.cin) + 2 * aj - 1) // (2 * aj), wgrad_split(L, rows, num_cus),
                  (groups + rchunk // 8 - 1) // (rchunk // 8))


def case_launches(name, form="dense", num_cus=NUM_CUS):
    """(the wgrad_bf16x3_kernel launches of one backward of a case, the layers that stay on the fp32 kernels)."""
    params = case_shape(name)[0]
    rows = case_rows(name, form)
    ls = layers(params)
    return [launch(L, rows, num_cus) for L in ls if gemm_form(L)], [L for L in ls if not gemm_form(L)]


def row_key(l):
    """The profile row of a launch under HIFICAR_PROFILE_DETAIL=1 without its split count: (text in front of " sS", text behind it)."""
    return f"wgrad_bf16x3_kernel<{l.aj},{l.rchunk}> {l.layer.cout}x{l.layer.cin}k1p1", "r1 n1"


def expected_rows(launches):
    """{(row without its split count): (launches, split count)}."""
    out = {}
    for l in launches:
        k = row_key(l)
        n, s = out.get(k, (0, l.nsplit))
        assert s == l.nsplit
        out[k] = (n + 1, s)
    return out


def parse_row(row):
    """'kernel<..> CxIkKpP sS rR nN' -> (kernel with instantiation, (cout, cin, K), S, (text in front of sS, text behind it))."""
    kernel, shape, s, r, n = row.split(" ")
    cout, rest = shape.split("x")
    cin, rest = rest.split("k")
    K = rest.split("p")[0]
    return kernel, (int(cout), int(cin), int(K)), int(s[1:]), (kernel + " " + shape, r + " " + n)


# ------------------------------------------------------------------------------------------------ the split pass
def bf16(a):
    """float32 array -> its bf16 bits, round to nearest even (finite values)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def split_rows_t(x, valid=None):
    """fp32 rows x [M][C] -> the bytes of [ceil(M / 8)][C][hi 8 | lo 8] bf16: hi = bf16(x), lo = bf16(x - hi); rows past M and rows that are
    not ``valid`` (bool [M]) are zero bits, whatever x holds there."""
    M, C = x.shape
    G = (M + 7) // 8
    xp = np.zeros((G * 8, C), dtype=np.float32)
    keep = np.ones(M, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    xp[:M][keep] = x[keep]
    hi = bf16(xp)
    lo = bf16(xp - (hi.astype(np.uint32) << 16).view(np.float32))
    out = np.stack([hi.reshape(G, 8, C).transpose(0, 2, 1), lo.reshape(G, 8, C).transpose(0, 2, 1)], axis=2)  # (G, C, 2, 8)
    return np.ascontiguousarray(out).view(np.uint8).reshape(-1)
