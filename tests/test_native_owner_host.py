"""``articulatory_amd._owner`` without a GPU: ``NativeOwner``'s lifecycle on a minimal subclass and on every real owner, against a stub
library that records its calls (no double destroy or failed creation here ever reaches ``libhificar.so``); ``create_handle``, ``scratch``
and ``aligned`` on CPU tensors; and that the package keeps each shared idiom in one place."""

import copy
import ctypes
import gc
import os
import pickle
import re

import pytest
import torch

import articulatory_amd
from articulatory_amd import _native, _owner, features, losses, models
from articulatory_amd._owner import ABSENT, NativeOwner, aligned, create_handle, scratch
from articulatory_amd.utils import optim_hook
from test_hubert_host import TINY as HUBERT_TINY
from test_wavlm_host import TINY as WAVLM_TINY

MEL_KW = dict(fs=16000, fft_size=1024, hop_size=256, win_length=None, window="hann", num_mels=80, fmin=0, fmax=11025)  # tests/test_gpu_disc.py


class StubLib:
    """Every attribute is an entry point that records (name, arguments) and returns 0, or what ``results`` holds for its name: a value,
    or a list of values taken call by call."""

    def __init__(self, **results):
        self.calls, self.results = [], results

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            r = self.results.get(name, 0)
            return r.pop(0) if isinstance(r, list) else r

        return entry

    def __reduce__(self):
        raise TypeError("a library object is never copied or pickled")

    def named(self, name):
        return [args for n, args in self.calls if n == name]


class Tiny(NativeOwner, torch.nn.Module):
    """The smallest owner: a destroy entry point, one cache of each idle kind, and a ``_native_handle`` over ``create_handle``."""

    _DESTROY = "tiny_destroy"
    _ENGINE = "tiny_engine"
    _NATIVE = {"_handle": None, "_cache": {}, "_flag": False, "_note": ABSENT}
    _PROCESS = {"_lib": None, "_wiring": None}

    def __init__(self, lib=None):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.arange(6.0).reshape(2, 3))
        self.kept = 7
        self._reset_native()
        self._stub = lib

    def _native_handle(self, finalize=lambda h: None):
        if self._handle is None:
            self._lib = self._stub
            state = {"a": torch.zeros(2, 3), "b": torch.zeros(4), "c": torch.zeros(1)}
            self._handle = create_handle(self._lib, "tiny", lambda h: self._lib.tiny_create(h), state, finalize)
        return self._handle


OWNERS = {
    "Tiny": Tiny,
    "HiFiGANGenerator": lambda: models.HiFiGANGenerator(in_channels=13, channels=64, use_ar=False),
    "GBlockGenerator": lambda: models.GBlockGenerator(in_channels=13, channels=64, g_scales=[5, 1, 4, 1, 1, 2, 1, 2, 1, 1], g_kernel_sizes=[3] * 10,
                                                      use_ar=False),
    "Discriminator": lambda: models.HiFiGANMultiScaleMultiPeriodDiscriminator(scales=1, periods=[2]),
    "BiGRU": lambda: models.BiGRU(in_channels=8, hidden_size=64, out_channels=12),
    "Transformer": lambda: models.Transformer(in_channels=12, out_channels=8, elayers=1, hidden_dim=128),
    "HuBERT": lambda: features.HuBERT(HUBERT_TINY),
    "WavLM": lambda: features.WavLM(WAVLM_TINY),
    "MFCC": features.MFCC,
    "LogMel": lambda: features.LogMel(16000),
    "LinearHead": lambda: features.LinearHead(torch.randn(3, 16).numpy(), torch.randn(3).numpy()),
    "MelSpectrogramLoss": lambda: losses.MelSpectrogramLoss(**MEL_KW),
    "STFTLoss": losses.STFTLoss,
}
DESTROY = dict(Tiny="tiny_destroy", HiFiGANGenerator="hificar_destroy", GBlockGenerator="hificar_destroy", Discriminator="hificar_disc_destroy",
               BiGRU="hificar_bigru_destroy", Transformer="hificar_xfmr_destroy", HuBERT="hificar_hubert_destroy", WavLM="hificar_hubert_destroy",
               MFCC="hificar_feat_destroy", LogMel="hificar_feat_destroy", LinearHead="hificar_linear_destroy",
               MelSpectrogramLoss="hificar_mel_destroy", STFTLoss="hificar_mel_destroy")
WATCHED = ("HiFiGANGenerator", "GBlockGenerator", "Discriminator", "BiGRU", "Transformer", "HuBERT", "WavLM")


def busy_value(idle):
    """Something a field can hold in the middle of everything: never its idle value."""
    if idle is False:
        return True
    return {"k": 1} if isinstance(idle, dict) else ("busy",)


def make_busy(m):
    """``m`` with a handle, the stub library and every field of both tables set by hand; returns (stub, handle, {field: value})."""
    lib, handle = StubLib(), ctypes.c_void_p(1)
    held = {k: busy_value(v) for k, v in {**m._NATIVE, **m._PROCESS}.items()}
    held.update(_handle=handle, _lib=lib)
    m.__dict__.update(held)
    return lib, handle, held


def assert_idle(m, table):
    for k, idle in table.items():
        if idle is ABSENT:
            assert k not in m.__dict__, k
        elif isinstance(idle, dict):
            assert m.__dict__[k] == idle and m.__dict__[k] is not idle, k  # a fresh object per instance, never the table's own
        else:
            assert m.__dict__[k] is idle, k


def test_the_tables_name_what_each_owner_held_before():
    """The per-process fields of the owners, as their hand-written lists had them: a field dropped from a table would travel with a copy."""
    for name, want in dict(
            HiFiGANGenerator={"_handle", "_lib", "_workspace_buf", "_grad_slots", "_grad_sync", "_param_sig", "_plist_cache", "_plist_epoch",
                              "_raw_cache", "_sent_sig", "_sent_held", "_raw_cnames"},
            Discriminator={"_handle", "_lib", "_grad_sync", "_info_cache", "_sent_sig", "_sent_held", "_raw_cnames", "_real_cache", "_early_real",
                           "_gside_done", "_raw_cache", "_early_stream"},
            BiGRU={"_handle", "_lib", "_workspace_buf", "_sig", "_train_ws_buf", "_lens", "_on_device", "_dirty", "_grad_info", "_low"},
            Transformer={"_handle", "_lib", "_workspace_buf", "_sig", "_train_ws_buf", "_lens", "_on_device", "_dirty", "_grad_info", "_packed",
                         "_last_stats"},
            MFCC={"_handle", "_lib", "_handle_dev", "_workspace_buf"}, LinearHead={"_handle", "_lib", "_handle_key", "_workspace_buf"},
            STFTLoss={"_handle", "_lib"}).items():
        m = OWNERS[name]()
        assert set(m._NATIVE) | set(m._PROCESS) == want, name
        assert not set(m._NATIVE) & set(m._PROCESS), name
        assert m._DESTROY == DESTROY[name]


@pytest.mark.parametrize("name", list(OWNERS))
def test_invalidate_destroys_the_handle_exactly_once(name):
    """``_invalidate()`` calls the class's destroy entry point once, with the handle it held; a second one and a later ``__del__`` call
    nothing.  Every handle-bound field (``_NATIVE``) is idle afterwards; what outlives a handle (``_PROCESS``: the library object, the
    gradient-sync wiring, a training forward's transient fields) stays as it was, which is what each owner's own ``_invalidate`` did."""
    m = OWNERS[name]()
    assert_idle(m, m._NATIVE)
    assert_idle(m, m._PROCESS)
    lib, handle, held = make_busy(m)
    m._invalidate()
    assert [(n, a[0]) for n, a in lib.calls] == [(DESTROY[name], handle)] and lib.calls[0][1][0] is handle
    assert_idle(m, m._NATIVE)
    for k in m._PROCESS:
        assert m.__dict__[k] is held[k], k
    m._invalidate()
    m.__del__()
    assert len(lib.calls) == 1
    m._reset_native()
    assert_idle(m, m._PROCESS)


@pytest.mark.parametrize("name", list(OWNERS))
def test_del_of_a_half_constructed_owner_raises_nothing(name):
    cls = type(OWNERS[name]())
    bare = cls.__new__(cls)  # no __init__: neither _handle nor _lib exists
    bare.__dict__.pop("_handle", None)
    assert "_handle" not in bare.__dict__ and "_lib" not in bare.__dict__
    bare.__del__()
    bare._invalidate()
    half = cls.__new__(cls)
    half.__dict__["_handle"], half.__dict__["_lib"] = ctypes.c_void_p(1), None  # a handle but no library to destroy it with
    half.__del__()
    assert half.__dict__["_handle"] is None


def clones_of(m):
    return copy.deepcopy(m), pickle.loads(pickle.dumps(m))


@pytest.mark.parametrize("name", list(OWNERS))
def test_copies_and_pickles_in_the_middle_of_everything_come_back_idle(name):
    """A clone carries no field of either table (neither the handle nor the stub library can be copied or pickled at all), shares no mutable
    idle value with the original or the class, keeps the module's own state, and is watched where the class is; the original keeps what it
    held."""
    m = OWNERS[name]()
    lib, handle, held = make_busy(m)
    for clone in clones_of(m):
        assert_idle(clone, clone._NATIVE)
        assert_idle(clone, clone._PROCESS)
        for k, v in held.items():
            assert k not in clone.__dict__ or clone.__dict__[k] is not v, k
        assert all(torch.equal(a, b) and a is not b for a, b in zip(m.state_dict().values(), clone.state_dict().values()))
        assert (clone in optim_hook._watched) == (name in WATCHED)
        if name == "Tiny":
            assert clone.kept == 7
    for k, v in held.items():
        assert m.__dict__[k] is v, k
    assert lib.calls == []
    m.__dict__["_handle"] = None  # (made up: nothing to destroy)


def test_the_losses_can_be_copied_and_pickled_after_use():
    """``MelSpectrogramLoss``, ``STFTLoss`` and ``MultiResolutionSTFTLoss`` with a handle: before they shared ``NativeOwner`` they had no
    ``__getstate__``, and ``copy.deepcopy`` / ``pickle.dumps`` of a used criterion raised ``ValueError: ctypes objects containing pointers
    cannot be pickled``.  A clone has the configuration and no handle; the container's clones hold clones of its resolutions."""
    mel, multi = losses.MelSpectrogramLoss(**MEL_KW), losses.MultiResolutionSTFTLoss()
    stubs = [make_busy(f)[0] for f in [mel, *multi.stft_losses]]
    for clone in clones_of(mel):
        assert clone._handle is None and clone._lib is None and clone._cfg.num_mels == 80 and (clone.melmat == mel.melmat).all()
    for clone in clones_of(multi):
        assert [f._cfg.fft_size for f in clone.stft_losses] == [1024, 2048, 512]
        for f, g in zip(clone.stft_losses, multi.stft_losses):
            assert f is not g and f._handle is None and f._lib is None and g._handle is not None
    assert all(s.calls == [] for s in stubs)
    for f in [mel, *multi.stft_losses]:
        f.__dict__["_handle"] = None


@pytest.mark.parametrize("name", list(OWNERS))
def test_setstate_takes_both_earlier_conventions(name):
    """A state without the per-process keys (the generators' and discriminators' convention) and one that carries them as None (the feature
    models', the speech features' and the linear head's) both load to an idle owner; fields that are absent while idle stay absent."""
    m = OWNERS[name]()
    cls = type(m)
    missing = m.__getstate__()
    assert not (set(m._NATIVE) | set(m._PROCESS)) & set(missing)
    as_none = dict(missing, **{k: None for k in (*m._NATIVE, *m._PROCESS)})
    for state in (missing, as_none):
        new = cls.__new__(cls)
        new.__setstate__(dict(state))
        assert_idle(new, new._NATIVE)
        assert_idle(new, new._PROCESS)
        assert (new in optim_hook._watched) == (name in WATCHED)


def test_engine_creates_the_handle_first():
    lib = StubLib(tiny_engine=77)
    m = Tiny(lib)
    assert m.engine().value == 77 and [n for n, _ in lib.calls] == ["tiny_create", "tiny_set_weight", "tiny_set_weight", "tiny_set_weight", "tiny_engine"]
    with pytest.raises(RuntimeError, match="MFCC.engine: no native handle yet; run a forward first"):
        features.MFCC().engine()
    m._invalidate()


def test_create_handle_destroys_what_it_could_not_finish(monkeypatch):
    monkeypatch.setattr(_native, "load_library", lambda: StubLib(hificar_last_error=b"stub said no"))
    # every tensor set, finalize called, nothing destroyed
    lib = StubLib()
    m = Tiny(lib)
    seen = []
    handle = m._native_handle(seen.append)
    assert m._handle is handle and seen == [handle] and lib.named("tiny_destroy") == []
    sets = lib.named("tiny_set_weight")
    assert [(a[1], list(a[3]), a[4]) for a in sets] == [(b"a", [2, 3], 2), (b"b", [4], 1), (b"c", [1], 1)] and all(a[0] is handle for a in sets)
    m._invalidate()
    assert len(lib.named("tiny_destroy")) == 1
    # set_weight fails on the second tensor
    lib = StubLib(tiny_set_weight=[0, _native.E_INVALID, 0])
    m = Tiny(lib)
    with pytest.raises(ValueError, match="tiny_set_weight: stub said no"):
        m._native_handle(seen.append)
    assert len(lib.named("tiny_set_weight")) == 2 and len(lib.named("tiny_destroy")) == 1 and m._handle is None and len(seen) == 1
    assert lib.named("tiny_destroy")[0][0] is lib.named("tiny_create")[0][0]
    # finalize fails

    def refuse(h):
        raise RuntimeError("finalize said no")

    lib = StubLib()
    m = Tiny(lib)
    with pytest.raises(RuntimeError, match="finalize said no"):
        m._native_handle(refuse)
    assert len(lib.named("tiny_set_weight")) == 3 and len(lib.named("tiny_destroy")) == 1 and m._handle is None
    del m
    gc.collect()
    assert len(lib.named("tiny_destroy")) == 1


class Box:
    buf = None


def test_scratch_grows_only_and_keeps_to_its_device():
    cpu, meta = torch.device("cpu"), torch.device("meta")
    box, n = Box(), 1000
    ptr, nbytes = scratch(box, "buf", n, cpu)
    first = box.buf
    assert first.numel() == n + 256 and first.dtype == torch.uint8
    assert ptr % 256 == 0 and 0 <= ptr - first.data_ptr() < 256 and nbytes == first.numel() - (ptr - first.data_ptr()) >= n
    assert scratch(box, "buf", 10, cpu) == (ptr, nbytes) and box.buf is first  # a smaller request: the same tensor
    assert scratch(box, "buf", n, lambda: meta) == (ptr, nbytes) and box.buf is first  # (a callable is asked only to allocate)
    ptr2, nbytes2 = scratch(box, "buf", n + 1, cpu)
    grown = box.buf
    assert grown is not first and grown.numel() == int((n + 1 + 256) * 1.25)
    assert ptr2 % 256 == 0 and nbytes2 == grown.numel() - (ptr2 - grown.data_ptr())
    scratch(box, "buf", 10, meta)  # the buffer sits on another device: replaced
    assert box.buf is not grown and box.buf.device == meta
    asked = []
    other = Box()
    scratch(other, "buf", 5, lambda: asked.append(1) or cpu)
    scratch(other, "buf", 5, lambda: asked.append(1) or cpu)
    assert asked == [1] and other.buf.numel() == 261


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("nbytes", [0, 1, 255, 256, 4097])
def test_aligned_leaves_the_bytes_asked_for_behind_its_pointer(nbytes, dtype):
    t, ptr = aligned(nbytes, "cpu", dtype)
    end = t.data_ptr() + t.numel() * t.element_size()
    assert t.dtype == dtype and t.numel() == nbytes // t.element_size() + 256 // t.element_size()  # the sizes the call sites had
    assert ptr % 256 == 0 and t.data_ptr() <= ptr and end - ptr >= nbytes


def test_each_shared_idiom_is_written_once():
    root = os.path.dirname(articulatory_amd.__file__)
    found = {"del": [], "align": [], "stream": []}
    for folder, _, files in os.walk(root):
        for f in files:
            if not f.endswith(".py"):
                continue
            path = os.path.join(folder, f)
            for line in open(path):
                code = line.split("#")[0]
                if re.search(r"def __del__|__del__\s*=", code):
                    found["del"].append(path)
                if "% 256" in code:
                    found["align"].append(path)
                if "current_stream().cuda_stream" in code:
                    found["stream"].append(path)
    assert found == {k: [_owner.__file__] for k in found}, found
