"""Host side of streaming synthesis (articulatory_amd/streaming.py, C ABI hificar_ar_step) without a GPU: the session bookkeeping
driven with a fake native step, and the entry point's argument checks on a created (not finalized) handle."""

import ctypes

import numpy as np
import pytest

from conftest import E2W_PARAMS
from articulatory_amd import _native
from articulatory_amd.streaming import StreamSchedule

HOP = 80


class FakeNative:
    """Stands in for hificar_ar_step: records every table and returns sample values that name (row, frame, sample)."""

    def __init__(self, chunk):
        self.chunk = chunk
        self.tables = []

    def __call__(self, table):
        assert table.dtype == np.int32 and table.shape[1] == 4
        self.tables.append(table.copy())
        out = np.full((table.shape[0], HOP * self.chunk), -1.0)
        for b, (row, col, valid, first) in enumerate(table):
            out[b, :HOP * valid] = np.arange(HOP * valid) + 1000.0 * col + 1e6 * row
        return out


def test_step_table_for_staggered_sessions():
    s = StreamSchedule(4, 25, 4)
    fake = FakeNative(25)
    a = s.open()
    a_frames = s.push(a, 30)
    assert a_frames == [(0, 0, 30)]
    assert s.step(fake, HOP).keys() == {a}
    b = s.open()
    s.push(b, 10)
    s.push(a, 20)  # a: 25 buffered; b: 10 (not ready)
    out = s.step(fake, HOP)
    assert out.keys() == {a}
    s.push(b, 15)
    s.push(a, 3)
    out = s.step(fake, HOP)
    assert list(out) == [b]  # a has 3 frames only: waits for more
    assert [t.tolist() for t in fake.tables] == [[[0, 0, 25, 1]], [[0, 25, 25, 0]], [[1, 0, 25, 1]]]
    s.push(b, 25)
    s.push(a, 22)
    s.step(fake, HOP)
    assert fake.tables[-1].tolist() == [[0, 50, 25, 0], [1, 25, 25, 0]]  # in opening order
    assert len(out[b]) == HOP * 25


def test_ring_placement_and_a_push_that_wraps():
    s = StreamSchedule(2, 10, 3)  # 30-frame ring
    fake = FakeNative(10)
    a = s.open()
    assert s.push(a, 25) == [(0, 0, 25)]
    s.step(fake, HOP)
    s.step(fake, HOP)  # consumed 20: 5 buffered
    assert s.push(a, 20) == [(25, 0, 5), (0, 5, 15)]  # wraps at the ring's end
    out = s.step(fake, HOP)
    assert fake.tables[-1].tolist() == [[0, 20, 10, 0]]
    s.step(fake, HOP)
    assert fake.tables[-1].tolist() == [[0, 0, 10, 0]]  # the chunk of frames 30..39 starts at column 0: chunks never wrap
    assert out[a][0] == 1000.0 * 20


def test_final_short_chunk_and_zero_frame_flush():
    s = StreamSchedule(2, 25, 4)
    fake = FakeNative(25)
    a = s.open()
    s.push(a, 60)
    s.flush(a)
    lens = []
    while s.is_open(a):
        out = s.step(fake, HOP)
        lens.append(len(out[a]))
    assert lens == [HOP * 25, HOP * 25, HOP * 10]
    assert fake.tables[-1].tolist() == [[0, 50, 10, 0]]
    with pytest.raises(KeyError):
        s.push(a, 1)  # closed itself after its final chunk
    b = s.open()
    s.flush(b)  # nothing pushed: closed at once, nothing to synthesise
    assert not s.is_open(b)
    assert s.step(fake, HOP) == {}
    c = s.open()
    s.push(c, 25)
    s.push(c, 0)
    s.step(fake, HOP)
    assert s.is_open(c)
    s.flush(c)  # a whole number of chunks: nothing left, closes at the flush
    assert not s.is_open(c)


def test_row_reuse_sets_the_first_chunk_flag():
    s = StreamSchedule(2, 5, 2)
    fake = FakeNative(5)
    a, b = s.open(), s.open()
    assert (s.row(a), s.row(b)) == (0, 1)
    with pytest.raises(RuntimeError, match="in use"):
        s.open()
    s.push(a, 7)
    s.push(b, 5)
    s.step(fake, HOP)
    s.close(a)  # abandoned with 2 frames buffered
    c = s.open()
    assert c not in (a, b) and s.row(c) == 0  # the lowest free row, a new id
    s.push(c, 5)
    s.push(b, 5)
    s.step(fake, HOP)
    assert fake.tables[-1].tolist() == [[1, 5, 5, 0], [0, 0, 5, 1]]  # b continues; c starts fresh at column 0 with the flag set


def test_back_pressure_and_bad_ids():
    s = StreamSchedule(2, 10, 2)
    fake = FakeNative(10)
    a = s.open()
    s.push(a, 20)
    with pytest.raises(RuntimeError, match="step"):
        s.push(a, 1)
    assert s.buffered(a) == 20  # a refused push changes nothing
    s.step(fake, HOP)
    s.push(a, 10)
    with pytest.raises(ValueError):
        s.push(a, -1)
    s.flush(a)
    with pytest.raises(RuntimeError, match="flushed"):
        s.push(a, 1)
    with pytest.raises(KeyError):
        s.push(12345, 1)
    b = s.open()
    s.close(b)
    with pytest.raises(KeyError):
        s.close(b)
    with pytest.raises(KeyError):
        s.flush(b)


def test_nothing_ready_makes_no_native_call():
    s = StreamSchedule(3, 25, 4)

    def boom(table):
        raise AssertionError("native step called with nothing ready")

    assert s.step(boom, HOP) == {}
    a = s.open()
    s.push(a, 24)
    assert s.step(boom, HOP) == {}
    b = s.open()
    s.flush(b)
    assert s.step(boom, HOP) == {}


def test_a_failing_native_step_changes_no_state():
    s = StreamSchedule(1, 5, 2)
    a = s.open()
    s.push(a, 5)

    def fail(table):
        raise RuntimeError("device error")

    with pytest.raises(RuntimeError):
        s.step(fail, HOP)
    assert s.plan() == [(a, (0, 0, 5, 1))]


# ---- the C entry point's host-side checks (no device work: the handle is created but never finalized) -------------------------------
@pytest.fixture(scope="module")
def lib():
    return _native.load_library()


def _handle(lib, **over):
    p = dict(E2W_PARAMS, use_tanh=True)
    p.update(over)
    cfg = _native.make_config(p, _native.PREC_F32)
    h = ctypes.c_void_p()
    assert lib.hificar_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, lib.hificar_last_error()
    return h


def _step(lib, h, table, chunk=25, ctx_rows=4, c_cstride=100):
    t = np.ascontiguousarray(table, dtype=np.int32).reshape(-1, 4)
    dummy = ctypes.c_void_p(256)  # never dereferenced: every check here fails before anything is enqueued
    return lib.hificar_ar_step(h, dummy, 13 * c_cstride, c_cstride, t.ctypes.data_as(ctypes.c_void_p), t.shape[0], chunk, dummy,
                               ctx_rows, dummy, dummy, 1 << 30, None)


def test_cabi_argument_checks(lib):
    h = _handle(lib)
    try:
        def err(table, **kw):
            rc = _step(lib, h, table, **kw)
            return rc, lib.hificar_last_error().decode()

        rc, msg = err([[4, 0, 25, 1]])
        assert rc == -1 and "row 4 outside [0, 4)" in msg
        rc, msg = err([[-1, 0, 25, 1]])
        assert rc == -1 and "outside" in msg
        rc, msg = err([[1, 0, 25, 1], [1, 25, 25, 0]])
        assert rc == -1 and "appears twice" in msg
        rc, msg = err([[0, 0, 0, 1]])
        assert rc == -1 and "valid frames 0 outside [1, 25]" in msg
        rc, msg = err([[0, 0, 26, 1]])
        assert rc == -1 and "valid frames 26" in msg
        rc, msg = err([[0, 90, 25, 1]])
        assert rc == -1 and "feature rows" in msg
        rc, msg = err([[0, 0, 6, 1]], chunk=6)  # 6 frames x 80 = 480 samples < ar_input 512
        assert rc == -1 and "ar_input (512) > chunk audio length (480)" in msg
        rc, msg = err([[0, 0, 25, 1]] * 5, ctx_rows=4)
        assert rc == -1
        assert lib.hificar_ar_step(h, None, 0, 1, None, 1, 25, None, 4, None, None, 0, None) == -1
        assert "null argument" in lib.hificar_last_error().decode()
        # a well-formed table reaches the state check: the model has not been finalized
        rc, msg = err([[0, 0, 25, 1], [3, 50, 10, 0]])
        assert rc == -2 and "finalize" in msg
    finally:
        lib.hificar_destroy(h)


@pytest.mark.parametrize("over,msg", [
    (dict(use_ar=False, in_channels=13), "use_ar=false"),
    (dict(use_spk_id=True, num_spk=4, spk_emb_size=8), "conditioned"),
])
def test_cabi_refuses_models_it_does_not_stream(lib, over, msg):
    h = _handle(lib, **over)
    try:
        assert _step(lib, h, [[0, 0, 25, 1]]) == -1
        assert msg in lib.hificar_last_error().decode()
    finally:
        lib.hificar_destroy(h)
