"""The shapes of the packed Transformer training suite (tests/test_transformer_packed_host.py, tests/test_gpu_transformer_packed.py): every
``transformer_ragged_oracle.RAGGED_SHAPES`` entry plus two whose boundaries only matter to the packed row layout, drawn exactly as
``ragged_case`` draws.  The packed step computes the ragged step's function, so the restatement, its gate handling and the bars are those of
tests/transformer_ragged_oracle.py, used as they stand.  Test infrastructure only: no file of the package imports it.
"""

import contextlib
from collections import OrderedDict

import transformer_ragged_oracle as R

# name -> (model params, B, T, lengths, dropout p), as RAGGED_SHAPES
PACKED_SHAPES = OrderedDict([
    # eight boundaries inside one conv row tile and one column-sum chunk, an empty and two full sequences
    ("many", (R.BASE, 8, 40, (40, 1, 0, 7, 39, 2, 40, 13), 0.2)),
    # row0 = 0, 128, 256: a gap row is the last row of chunk 0, a sequence starts on a chunk edge, Mp = 512
    ("edge256", (R.BASE, 3, 127, (127, 127, 60), 0.2)),
])
# (admitted under the rule of RAGGED_SEEDS' comments: change a seed, never a bar; neither had to change)
PACKED_SEEDS = dict(many=8700, edge256=8701)
ALL_SHAPES = OrderedDict(list(R.RAGGED_SHAPES.items()) + list(PACKED_SHAPES.items()))
GRANULE = 256  # Mp is a multiple of it (include/hificar.h: hificar_xfmr_packed_rows)


@contextlib.contextmanager
def _extended():
    """The oracle module's tables with the two packed shapes, for the length of one call: other test modules see them unchanged."""
    saved = R.RAGGED_SHAPES, R.RAGGED_SEEDS
    R.RAGGED_SHAPES, R.RAGGED_SEEDS = ALL_SHAPES, dict(saved[1], **PACKED_SEEDS)
    try:
        yield
    finally:
        R.RAGGED_SHAPES, R.RAGGED_SEEDS = saved


def packed_case(name, step=0):
    """``ragged_case`` over ALL_SHAPES."""
    with _extended():
        return R.ragged_case(name, step)


def packed_restatement(name, dtype, device="cpu", gates=None):
    """``ragged_restatement`` over ALL_SHAPES."""
    with _extended():
        return R.ragged_restatement(name, dtype, device=device, gates=gates)


def seed_of(name):
    return PACKED_SEEDS[name] if name in PACKED_SEEDS else R.RAGGED_SEEDS[name]


def packed_rows(lengths):
    """Mp by the issue's formula: every sequence's frames and one gap row each, rounded up to the granule."""
    return -(-(sum(lengths) + len(lengths)) // GRANULE) * GRANULE
