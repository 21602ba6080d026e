"""The C-ABI library loads and exports every symbol include/hificar.h declares; host-only entry points
(create / set_weight / workspace_bytes / macs / error reporting) behave.  No compute calls: no GPU here."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import E2W_PARAMS, REPO
from articulatory_amd import _native


@pytest.fixture(scope="module")
def lib():
    return _native.load_library()


def _full_params(**over):
    p = dict(E2W_PARAMS, use_tanh=True)
    p.update(over)
    return p


def test_exports_every_declared_symbol(lib):
    hdr = open(os.path.join(REPO, "include", "hificar.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(hificar_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_native.SYMBOLS)
    for sym in declared:
        assert hasattr(lib, sym), sym
    assert b"gfx950" in lib.hificar_version()


def test_config_struct_matches_header_layout():
    # 5 scalars + 8 + 8 + 1 + 4 + 4 + 16 + 2 ints + float + 6 ints + 7 conditioning ints = 63 x 4 bytes
    assert ctypes.sizeof(_native.HificarConfig) == 4 * (5 + 8 + 8 + 1 + 4 + 4 + 16 + 2 + 1 + 6 + 7)
    assert ctypes.sizeof(_native.HificarKernelStat) == 96 + 8 + 3 * 8


def test_training_structs_match_header_layout():
    """The constants the discriminator and GBlock structs are sized by, against the header's text."""
    assert _native.DISC_MAX_SUBS == 8 and _native.DISC_MAX_LAYERS == 12  # HIFICAR_DISC_MAX_* of the header
    hdr = open(os.path.join(REPO, "include", "hificar.h")).read()
    assert "#define HIFICAR_DISC_MAX_SUBS 8" in hdr and "#define HIFICAR_DISC_MAX_LAYERS 12" in hdr
    assert _native.MAX_GBLOCKS == 10 and "#define HIFICAR_MAX_GBLOCKS 10" in hdr


def _header_text():
    """include/hificar.h without its comments: what the tests below read on their own, not through _native.parse_header."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "hificar.h")).read(), flags=re.S)


HEADER_STRUCTS = re.findall(r"typedef\s+struct\s+(\w+)\s*\{", _header_text())  # every struct with a body: a new one is covered the day it is added


def test_every_struct_of_the_header_is_enumerated():
    assert len(HEADER_STRUCTS) >= 10 and {"hificar_config", "hificar_kernel_stat", "hificar_feat_config"} <= set(HEADER_STRUCTS)
    assert set(HEADER_STRUCTS) == set(_native.STRUCTS)


@pytest.mark.parametrize("cname", HEADER_STRUCTS)
def test_struct_matches_header_layout(cname, tmp_path):
    """The C compiler's view of include/hificar.h against the ctypes class: the struct's size, and the offset and size of every field."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cls = _native.STRUCTS[cname]
    assert issubclass(cls, ctypes.Structure) and getattr(_native, cls.__name__) is cls
    fields = [f[0] for f in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hificar.h"\nint main(void) {\n'
                   f'  printf("%zu\\n", sizeof({cname}));\n' +
                   "".join(f'  printf("%zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));\n' for f in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(cls)]
    for f in fields:
        want += [getattr(cls, f).offset, getattr(cls, f).size]
    assert got == want


# ------------------------------------------------------------------------------------------------ prototypes
# Written out by hand from the header's text, not read from the parser: between them every scalar class (int, size_t, int64_t, uint64_t,
# float, double), every return class (int, size_t, int64_t, double, pointer, const char*, void) and every pointer rule.
_vp, _ci, _cs, _c64, _u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_int64, ctypes.c_uint64
_P = ctypes.POINTER
ANCHORS = {
    "hificar_forward": (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, _vp, _cs, _vp]),
    "hificar_bigru_forward_train": (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, ctypes.c_float, _u64, _u64, _vp, _cs, _vp, _cs, _vp]),
    "hificar_macs": (ctypes.c_double, [_vp, _ci, _ci]),
    "hificar_grad_floats": (_c64, [_vp]),
    "hificar_workspace_bytes": (_cs, [_vp, _ci, _ci]),
    "hificar_bigru_engine": (_vp, [_vp]),
    "hificar_disc_param_info": (_ci, [_vp, _ci, ctypes.c_char_p, _P(_c64), _P(_ci), _P(_c64)]),  # char*, int64_t*, int*
    "hificar_set_parameters_device": (_ci, [_vp, _P(ctypes.c_char_p), _P(_vp), _ci, _vp]),  # const char* const*, const float* const*
    "hificar_set_weight": (_ci, [_vp, ctypes.c_char_p, _vp, _P(_c64), _ci]),  # const char*, const int64_t*
    "hificar_ar_step": (_ci, [_vp, _vp, _c64, _c64, _vp, _ci, _ci, _vp, _ci, _vp, _vp, _cs, _vp]),  # int64_t by value
    "hificar_create": (_ci, [_P(_native.HificarConfig), _P(_vp)]),  # a header struct, a handle**
    "hificar_profile_end": (_ci, [_vp, _P(_native.HificarKernelStat), _ci, _P(_ci)]),
    "hificar_set_bucket_callback": (_ci, [_vp, _native.BUCKET_FN, _vp]),
    "hificar_debug_pack16": (_ci, [_ci, _ci, _ci, _ci, _ci, _ci, _vp, _vp, _cs, _P(_cs)]),  # uint16_t*, size_t*
    "hificar_pcm16": (_ci, [_vp, _vp, _cs, _vp]),  # int16_t*
    "hificar_last_error": (ctypes.c_char_p, []),
    "hificar_destroy": (None, [_vp]),
}


@pytest.mark.parametrize("name", sorted(ANCHORS))
def test_anchor_prototypes(lib, name):
    restype, argtypes = ANCHORS[name]
    fn = getattr(lib, name)
    assert fn.restype is restype
    assert len(fn.argtypes) == len(argtypes)
    for i, (got, want) in enumerate(zip(fn.argtypes, argtypes)):
        assert got is want, (name, i, got, want)


def test_every_symbol_has_a_complete_prototype(lib):
    """Parameter counts from a deliberately naive reading of the header (the text between a function's parentheses, split on commas), and a
    non-default restype wherever the header's return type is not int."""
    naive = re.findall(r"([\w \*]+?)\b(hificar_\w+)\s*\(([^()]*)\)\s*;", _header_text())
    assert len(naive) == len(_native.SYMBOLS) and {n for _, n, _ in naive} == set(_native.SYMBOLS)
    for ret, name, params in naive:
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name
        assert len(fn.argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), name
        assert (fn.restype is ctypes.c_int) == (ret.strip() == "int"), (name, ret, fn.restype)
        if "*" in ret:
            assert fn.restype in (ctypes.c_void_p, ctypes.c_char_p), (name, ret, fn.restype)


GOOD_HEADER = """/* a comment
over two lines */
#define T_N 3
#define T_NEG (-2)
typedef struct t_handle t_handle;
typedef struct t_cfg {
    int32_t a, b[T_N];
    float c[2][T_N];
    char name[8];
} t_cfg;
typedef void (*t_fn)(int i, void* user);
int t_create(const t_cfg* cfg, t_handle** out);
size_t t_bytes(const t_handle* h, int n, t_fn fn);
const char* t_error(void);
"""


def test_parser_reads_the_shapes_it_knows():
    fn = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_void_p)
    consts, structs, protos = _native.parse_header(GOOD_HEADER, callbacks={"t_fn": fn})
    assert consts == {"T_N": 3, "T_NEG": -2}
    cfg = structs["t_cfg"]
    assert cfg.__name__ == "TCfg" and [f[0] for f in cfg._fields_] == ["a", "b", "c", "name"]
    assert cfg._fields_[1][1] is ctypes.c_int32 * 3 and cfg._fields_[2][1] is (ctypes.c_float * 3) * 2 and cfg._fields_[3][1] is ctypes.c_char * 8
    assert protos == {"t_create": (ctypes.c_int, [ctypes.POINTER(cfg), ctypes.POINTER(ctypes.c_void_p)]),
                      "t_bytes": (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int, fn]), "t_error": (ctypes.c_char_p, [])}


@pytest.mark.parametrize("what,bad", [
    ("an unknown scalar type", "int t_f(long double x);"),
    ("an unsigned int is not an int", "int t_f(unsigned int x);"),
    ("an unknown struct pointer", "int t_f(t_other* p);"),
    ("a struct by value", "int t_f(t_cfg c);"),
    ("three levels of pointer", "int t_f(float*** p);"),
    ("an array extent naming an undefined macro", "typedef struct t_s { int a[T_UNDEFINED]; } t_s;"),
    ("an expression as array extent", "typedef struct t_s { int a[T_N + 1]; } t_s;"),
    ("a prototype without a parameter name", "int t_f(int, float* x);"),
    ("a pointer parameter without a name", "int t_f(const float*);"),
    ("a bit-field", "typedef struct t_s { int a : 3; } t_s;"),
    ("a pointer field", "typedef struct t_s { float* p; } t_s;"),
    ("an unknown field type", "typedef struct t_s { long a; } t_s;"),
    ("an unknown return type", "long t_f(int x);"),
    ("a function-pointer typedef without a CFUNCTYPE", "typedef void (*t_other_fn)(int i);"),
    ("a function-pointer typedef whose parameters are not its CFUNCTYPE's", "typedef void (*t_fn)(int i, void* user, void* more);"),
    ("a function-pointer parameter", "int t_f(void (*fn)(int), int x);"),
    ("a macro that is no integer", "#define T_X 1.5"),
    ("a declaration of no known shape", "enum t_e { T_A, T_B };"),
])
def test_parser_refuses_what_it_does_not_understand(what, bad):
    """Each of these raises, with the header line in the message; none of them yields a guessed int."""
    fn = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_void_p)
    line = GOOD_HEADER.count("\n") + 1
    with pytest.raises(_native.HeaderError, match=rf"^synthetic\.h:{line}: "):
        _native.parse_header(GOOD_HEADER + bad + "\n", path="synthetic.h", callbacks={"t_fn": fn})


def test_missing_header_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_native, "HEADER_PATH", str(tmp_path / "include" / "hificar.h"))
    with pytest.raises(RuntimeError, match=re.escape(str(tmp_path / "include" / "hificar.h"))):
        _native._parse_own_header()


def test_constants_come_from_the_header():
    for macro, value in re.findall(r"#define\s+HIFICAR_(\w+)\s+\(?(-?\d+)\)?", _header_text()):
        assert getattr(_native, macro) == int(value), macro
    assert _native.OK == 0 and _native.E_INVALID == -1 and _native.LOWRATE_MAX_FACTOR == 16 and _native.FEAT_MFCC == 1
    assert (_native.XFMR_HEADS, _native.XFMR_FF, _native.XFMR_REL) == (8, 3072, 100)  # not in the header: written out in the binding


def test_profile_rows_decodes_what_the_library_filled():
    """_native.profile_rows against a stand-in for the library: the rows it filled, at most `capacity` of them, and the count it reported."""
    class Lib:
        def __init__(self, n):
            self.n = n

        def hificar_profile_end(self, engine, stats, capacity, n_ref):
            assert engine == 7 and len(stats) == capacity
            for i in range(min(self.n, capacity)):
                stats[i].name, stats[i].launches, stats[i].total_ms, stats[i].flops, stats[i].bytes = b"k%d" % i, i + 1, 0.5 * i, 2.0 * i, 3.0 * i
            n_ref._obj.value = self.n
            return 0

    rows, n = _native.profile_rows(Lib(3), 7, 4)
    assert n == 3 and rows == [dict(name=f"k{i}", launches=i + 1, total_ms=0.5 * i, flops=2.0 * i, bytes=3.0 * i) for i in range(3)]
    rows, n = _native.profile_rows(Lib(6), 7, 4)
    assert n == 6 and [r["name"] for r in rows] == ["k0", "k1", "k2", "k3"]


def test_create_macs_workspace(lib):
    cfg = _native.make_config(_full_params(), _native.PREC_F32)
    h = ctypes.c_void_p()
    assert lib.hificar_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        mlp = 512 * 256 + 3 * 256 * 256 + 256 * 128
        # 117 668 864 conv MACs per frame (HiFi-CAR 13-dim) + 360 448 per PastFCEncoder call
        assert lib.hificar_macs(h, 1, 1) == 117668864 + mlp
        assert lib.hificar_macs(h, 64, 25) == 64 * (25 * 117668864 + mlp)
        assert abs(lib.hificar_macs(h, 1, 25) / 2000 - 1471041) < 1.0  # MAC per output sample at chunk 25
        ws = lib.hificar_workspace_bytes(h, 64, 25)
        assert 100e6 < ws < 200e6
        assert lib.hificar_workspace_bytes(h, 0, 25) == 0
        # forward before finalize is a state error, not a crash
        rc = lib.hificar_forward(h, 1, 1, 1, 1, 1, 1, 0, None)
        assert rc == -2 and b"finalize" in lib.hificar_last_error()
        rc = lib.hificar_finalize(h)
        assert rc == -2 and b"Missing key" in lib.hificar_last_error()
    finally:
        lib.hificar_destroy(h)


def test_set_weight_validation(lib):
    cfg = _native.make_config(_full_params(), _native.PREC_F32)
    h = ctypes.c_void_p()
    assert lib.hificar_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        w = np.zeros((512, 141, 7), dtype=np.float32)
        shp = (ctypes.c_int64 * 3)(512, 141, 7)
        assert lib.hificar_set_weight(h, b"input_conv.weight", w.ctypes.data, shp, 3) == 0
        bad = (ctypes.c_int64 * 3)(512, 140, 7)
        assert lib.hificar_set_weight(h, b"input_conv.weight", w.ctypes.data, bad, 3) == -1
        assert b"size mismatch for input_conv.weight" in lib.hificar_last_error()
        assert lib.hificar_set_weight(h, b"input_conv.weight_v", w.ctypes.data, shp, 3) == -1
        assert b"unexpected tensor name" in lib.hificar_last_error()
    finally:
        lib.hificar_destroy(h)


@pytest.mark.parametrize("over,msg", [
    (dict(out_channels=4), b"out_channels"),
    (dict(kernel_size=6), b"odd"),
    (dict(upsample_scales=[5, 4, 2, 2], upsample_kernel_sizes=[11, 8, 4, 4]), b"L_out"),
    (dict(channels=8), b"halvings"),
])
def test_create_rejects_unsupported(lib, over, msg):
    cfg = _native.make_config(_full_params(**over), _native.PREC_F32)
    h = ctypes.c_void_p()
    rc = lib.hificar_create(ctypes.byref(cfg), ctypes.byref(h))
    assert rc == -1
    assert msg in lib.hificar_last_error(), lib.hificar_last_error()


def test_create_accepts_four_blocks_and_single_conv_layers(lib):
    """Up to HIFICAR_MAX_BLOCKS = 4 residual blocks per stage (hifigan.py:134-145) and use_additional_convs = false (residual_block.py:191-205):
    accepted since round 5; a fifth block is refused before the C ABI is reached."""
    for over in (dict(resblock_kernel_sizes=[3, 7, 11, 13], resblock_dilations=[[1]] * 4), dict(use_additional_convs=False)):
        cfg = _native.make_config(_full_params(**over), _native.PREC_F32)
        h = ctypes.c_void_p()
        assert lib.hificar_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, lib.hificar_last_error()
        w = np.zeros((256, 256, 3), dtype=np.float32)
        shp = (ctypes.c_int64 * 3)(256, 256, 3)
        rc = lib.hificar_set_weight(h, b"blocks.0.convs2.0.1.weight", w.ctypes.data, shp, 3)
        assert rc == (0 if "resblock_kernel_sizes" in over else -1)  # no convs2 tensors without the additional convs
        lib.hificar_destroy(h)
    with pytest.raises(ValueError):
        _native.make_config(_full_params(resblock_kernel_sizes=[3, 5, 7, 9, 11], resblock_dilations=[[1]] * 5), _native.PREC_F32)


def test_create_accepts_any_width(lib):
    """The reference builds channels // 2**i wide stages for any `channels` (hifigan.py:108-145); widths below / between MFMA-tile
    multiples are padded to 32 channels internally (no compute call here: creation only needs no GPU)."""
    for channels in (64, 48, 100, 16):
        cfg = _native.make_config(_full_params(channels=channels), _native.PREC_F32)
        h = ctypes.c_void_p()
        assert lib.hificar_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, lib.hificar_last_error()
        lib.hificar_destroy(h)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "LIB_PATH", str(tmp_path / "libhificar.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.load_library()


def test_header_is_plain_c(tmp_path):
    """include/hificar.h is a C ABI: it must compile as C99 on its own (no C++ / HIP / torch types)."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    src = tmp_path / "t.c"
    src.write_text('#include "hificar.h"\nint main(void) { return hificar_version() == 0; }\n')
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
