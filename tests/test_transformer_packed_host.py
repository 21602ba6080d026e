"""Host-side checks of packed Transformer training (``pytest -m "not gpu"``): the admission of the two packed-specific shapes, the row count
``hificar_xfmr_packed_rows``, the new entry points of the C ABI, and the Python and trainer surface (``forward_padded(packed=True)``,
``pad_packed``).
"""

import ctypes
import os
import subprocess

import pytest
import torch

import transformer_packed_shapes as P
import transformer_ragged_oracle as R
import transformer_train_oracle as O
from conftest import REPO
from articulatory_amd import _native
from articulatory_amd.bin import train as T
from test_transformer_ragged_host import bigru_config, config

NEW_SYMBOLS = ("hificar_xfmr_packed_rows", "hificar_xfmr_tape_bytes_packed", "hificar_xfmr_train_workspace_bytes_packed",
               "hificar_xfmr_forward_train_packed", "hificar_xfmr_backward_packed")


@pytest.mark.parametrize("name", list(P.PACKED_SHAPES))
def test_packed_shape_is_admitted(name):
    """The rule of test_transformer_ragged_host.py::test_ragged_shape_is_admitted."""
    ref = P.packed_restatement(name, torch.float64)
    assert ref["kink"] > O.KINK_MARGIN
    worst = {k: e / bar for k, (e, bar) in O.errors(P.packed_restatement(name, torch.float32), ref).items()}
    k = max(worst, key=worst.get)
    print(f"{name}: worst fp32 share of a bar: {k} {worst[k]:.3f}; kink {ref['kink']:.3g}")
    assert worst[k] <= 0.5, (k, worst[k])


def test_shapes_are_the_issues_table_and_leave_the_ragged_tables_alone():
    assert [(k, v[1], v[2], v[3], v[4]) for k, v in P.PACKED_SHAPES.items()] == [
        ("many", 8, 40, (40, 1, 0, 7, 39, 2, 40, 13), 0.2), ("edge256", 3, 127, (127, 127, 60), 0.2)]
    assert all(v[0] == O.BASE for v in P.PACKED_SHAPES.values()) and P.PACKED_SEEDS == dict(many=8700, edge256=8701)
    before = list(R.RAGGED_SHAPES)
    P.packed_case("many")
    assert list(R.RAGGED_SHAPES) == before and "many" not in R.RAGGED_SEEDS
    # what the two shapes are for: row0 = 0, 128, 256 and Mp = 512; eight sequences inside one 256-row chunk
    assert P.packed_rows((127, 127, 60)) == 512 and P.packed_rows((40, 1, 0, 7, 39, 2, 40, 13)) == 256


def test_packed_rows_is_the_formula():
    lib = _native.load_library()

    def rows(lengths, B=None, T=None):
        arr = (ctypes.c_int32 * len(lengths))(*lengths)
        return lib.hificar_xfmr_packed_rows(len(lengths) if B is None else B, T, arr)

    for name, (_, B, T, lengths, _) in P.ALL_SHAPES.items():
        want = -(-(sum(lengths) + B) // 256) * 256
        assert rows(lengths, T=T) == want == P.packed_rows(lengths), name
    assert rows((5, -1), T=5) == 0 and rows((5, 6), T=5) == 0      # a negative length, a length above T
    assert rows((1, 0), T=5) == 0 and rows((0, 0), T=5) == 0       # fewer than two frames
    assert rows((2, 0), T=5) == 256 and rows((255,), T=255) == 256 and rows((256,), T=256) == 512 and rows((254, 0), T=254) == 256
    assert lib.hificar_xfmr_packed_rows(2, 5, None) == 0 and rows((5, 3), B=0, T=5) == 0 and rows((5, 3), T=0) == 0
    big = (700000,)  # Mp * 3072 >= 2^31
    assert rows(big, T=700000) == 0


def test_packed_entry_points_in_the_header_the_library_and_native(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hificar.h"\n'
                   "int use(hificar_xfmr* h, const float* x, float* y, void* p, const int32_t* n) {\n"
                   "    int mp = hificar_xfmr_packed_rows(2, 5, n);\n"
                   "    size_t tb = hificar_xfmr_tape_bytes_packed(h, 2, mp), wb = hificar_xfmr_train_workspace_bytes_packed(h, 2, mp);\n"
                   "    int rc = hificar_xfmr_forward_train_packed(h, x, n, n, y, y, 2, 5, 0.2f, 1u, 0u, p, tb, p, wb, 0);\n"
                   "    return rc ? rc : hificar_xfmr_backward_packed(h, x, n, 2, 5, p, tb, y, y, p, wb, 0);\n}\n")
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = _native.load_library()
    for sym in NEW_SYMBOLS:
        assert sym in _native.SYMBOLS and hasattr(lib, sym), sym
    text = open(os.path.join(REPO, "include", "hificar.h")).read()
    assert "Not built: packed (padding-free) GEMMs" not in text
    xfmr_not_built = [ln for ln in text.splitlines() if "Not built:" in ln and "multi-GPU training of this model" in ln]
    assert len(xfmr_not_built) == 1 and "packed" not in xfmr_not_built[0]
    # before finalize: the arguments are checked first, then the handle's state; the size queries answer 0
    h = ctypes.c_void_p()
    cfg = _native.make_xfmr_config(dict(O.BASE))
    _native.check(lib.hificar_xfmr_create(ctypes.byref(cfg), ctypes.byref(h)), "hificar_xfmr_create")
    try:
        def call(host, B=2, T=5):
            lens = (ctypes.c_int32 * len(host))(*host) if host is not None else None
            ptr = ctypes.cast(lens, ctypes.c_void_p) if host is not None else None
            return lib.hificar_xfmr_forward_train_packed(h, None, ptr, ptr, None, None, B, T, 0.0, 0, 0, None, 0, None, 0, None)

        E_INVALID, E_STATE = -1, -2  # include/hificar.h
        assert call((5, 3)) == E_STATE and b"hificar_xfmr_finalize" in lib.hificar_last_error()
        assert call(None) == E_INVALID and b"lengths_host" in lib.hificar_last_error()
        assert call((5, 6)) == E_INVALID and b"lengths[1]=6 outside [0, 5]" in lib.hificar_last_error()
        assert call((-1, 3)) == E_INVALID and b"lengths[0]=-1" in lib.hificar_last_error()
        assert call((1, 0)) == E_INVALID and b"sum of lengths = 1" in lib.hificar_last_error()
        assert call((2, 0)) == E_STATE
        assert lib.hificar_xfmr_tape_bytes_packed(h, 2, 256) == 0 and lib.hificar_xfmr_train_workspace_bytes_packed(h, 2, 256) == 0
        lens = (ctypes.c_int32 * 2)(5, 3)
        rc = lib.hificar_xfmr_backward_packed(h, None, ctypes.cast(lens, ctypes.c_void_p), 2, 5, None, 0, None, None, None, 0, None)
        assert rc == E_STATE and b"hificar_xfmr_finalize" in lib.hificar_last_error()
        assert lib.hificar_xfmr_backward_packed(h, None, None, 2, 5, None, 0, None, None, None, 0, None) == E_INVALID
    finally:
        lib.hificar_xfmr_destroy(h)


def test_forward_padded_packed_refuses_before_it_needs_a_device():
    from articulatory_amd.models import BiGRU, Transformer
    import inspect

    m = Transformer(**O.BASE).train()
    x = torch.zeros(2, 12, 5)
    with pytest.raises(RuntimeError, match="needs lengths"):
        m.forward_padded(x, None, packed=True)
    with pytest.raises(RuntimeError, match=r"lengths must lie in \[0, 5\]"):
        m.forward_padded(x, [5, 6], packed=True)
    with pytest.raises(RuntimeError, match="lengths has 3 entries for a batch of 2"):
        m.forward_padded(x, [5, 3, 1], packed=True)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        m.forward_padded(x, [5, 3], packed=True)
    assert m._calls == 0 and m._packed is False and m._lens is None
    with pytest.raises(RuntimeError, match="CUDA/HIP"):  # eval(): the flag has no effect, the call is forward(lengths=)
        m.eval().forward_padded(x, [5, 3], packed=True)
    assert "packed" not in inspect.signature(BiGRU.forward_padded).parameters


def test_inversion_trainer_builds_pad_packed_for_the_transformer_only():
    cpu = torch.device("cpu")
    tr = T.InversionTrainer(config(package_mode="pad_masked", pad_packed=True), cpu)
    assert tr.packed and tr.padded and not T.InversionTrainer(config(package_mode="pad_masked"), cpu).packed
    assert not T.InversionTrainer(config(package_mode="pad_masked", pad_packed=False), cpu).packed
    with pytest.raises(NotImplementedError, match=r"pad_packed.*Transformer.*pad_masked"):
        T.InversionTrainer(bigru_config(package_mode="pad_masked", pad_packed=True), cpu)
    with pytest.raises(NotImplementedError, match=r"pad_packed.*Transformer.*pad_masked"):
        T.InversionTrainer(bigru_config(package_mode="pad", pad_packed=True), cpu)
    with pytest.raises(NotImplementedError, match=r"pad_packed.*pad_masked"):
        T.InversionTrainer(config(pad_packed=True), cpu)  # random_window

    class Seen(Exception):
        pass

    def probe(x, lengths, packed=False):
        raise Seen((tuple(int(n) for n in lengths), packed))

    batch = {"x": torch.zeros(2, 12, 5), "y": torch.zeros(2, 8, 5), "lengths": torch.tensor([5, 3], dtype=torch.int32)}
    tr.G.forward_padded = probe
    tr.steps = 1
    with pytest.raises(Seen, match=r"\(\(5, 3\), True\)"):
        tr.train_step(batch)
