"""ctypes binding of libhificar.so, derived at import from its C ABI, include/hificar.h.

The header is the one place where an entry point, a struct or a constant is written down.  parse_header() reads its ``#define``s, its
``typedef struct``s and its prototypes; the constants (``HIFICAR_X`` -> ``X``), the ctypes.Structure classes (``hificar_x_config`` ->
``HificarXConfig``), SYMBOLS and every argtypes / restype of load_library() come from what it returns.  What the parser has no rule for it
refuses with the header line (HeaderError): it never guesses a type.

There is deliberately NO fallback: if the shared library is missing or a call fails, a
RuntimeError is raised.  The CPU oracle under ``oracle/`` is test infrastructure and is never
imported from here.
"""

import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# HIFICAR_LIB: developer override (A/B runs of two builds of the same ABI inside one gpurun call)
LIB_PATH = os.environ.get("HIFICAR_LIB") or os.path.join(_HERE, "libhificar.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "hificar.h"))  # in-tree only: there is no packaged copy

# hificar_bucket_fn (include/hificar.h): void (*)(int bucket, void* stream, void* user)
BUCKET_FN = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)


class HeaderError(RuntimeError):
    """The header holds a declaration the binding has no rule for."""


# by value, as a struct field, or (the first row of the pointer rules) behind a typed pointer
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "double": ctypes.c_double, "char": ctypes.c_char}
_TYPED_POINTEES = ("int", "int64_t", "size_t")  # small host arrays and results (shapes, counts, offsets): POINTER(T), ctypes checks the argument
_VOID_POINTEES = ("void", "float", "int32_t", "int16_t", "uint16_t")  # tensors, device or host: c_void_p, callers pass data_ptr() integers
_CLASS_NAMES = {"hificar_gblock_config": "HificarGBlockConfig"}  # where CamelCase of the C name is not the class's name


def parse_header(text, path="hificar.h", callbacks=None):
    """Plain-C99 header text -> (constants, structs, prototypes), each in the header's order:

    constants   macro name -> int, for every ``#define NAME <decimal integer>`` (parentheses allowed)
    structs     C name -> ctypes.Structure subclass, for every ``typedef struct name { ... } name;``
    prototypes  function name -> (restype, [argtypes])

    callbacks: function-pointer typedef name -> its CFUNCTYPE (default: hificar_bucket_fn).  Anything else — a type, a declarator, an array
    extent, a preprocessor line or a statement outside these shapes — raises HeaderError naming the line."""
    callbacks = {"hificar_bucket_fn": BUCKET_FN} if callbacks is None else callbacks

    def blank(m):  # keeps the line numbers
        return " " + "\n" * m.group().count("\n")

    def fail(pos, why):
        line = text.count("\n", 0, pos) + 1
        raise HeaderError(f"{path}:{line}: {why}")

    text = re.sub(r"/\*.*?\*/|//[^\n]*", blank, text, flags=re.S)
    text = re.sub(r"^#ifdef __cplusplus$.*?^#endif$", blank, text, flags=re.S | re.M)  # extern "C" { and its }

    constants = {}
    for m in re.finditer(r"^[ \t]*#[^\n]*$", text, flags=re.M):
        d = re.fullmatch(r"\s*#\s*define\s+(\w+)\s+\(?\s*(-?\d+)\s*\)?\s*", m.group())
        if d:
            constants[d.group(1)] = int(d.group(2))
        elif not re.fullmatch(r"\s*#\s*(ifndef\s+\w+|define\s+\w+|include\s*<\w+\.h>|endif)\s*", m.group()):
            fail(m.start(), f"preprocessor line outside '#define NAME <integer>': {m.group().strip()!r}")
    text = re.sub(r"^[ \t]*#[^\n]*$", blank, text, flags=re.M)

    structs, opaque, prototypes = {}, set(), {}

    def ctype(decl, pos, what, ret=False):
        """'const float* const*' and the like -> its ctypes type; a type outside these rules is refused."""
        m = re.fullmatch(r"(?:const )?(\w+) ?((?:\* ?(?:const ?)?)*)", decl.strip())
        base, stars = (m.group(1), m.group(2).count("*")) if m else (None, 0)
        if stars == 0:
            if base == "void" and ret:
                return None
            if base in _SCALARS:
                return _SCALARS[base]
            if base in callbacks:
                return callbacks[base]
        elif stars == 1:
            if base == "char":
                return ctypes.c_char_p
            if base in structs:
                return ctypes.POINTER(structs[base])
            if base in _TYPED_POINTEES:
                return ctypes.POINTER(_SCALARS[base])
            if base in _VOID_POINTEES or base in opaque:
                return ctypes.c_void_p
        elif stars == 2:
            if base == "char":
                return ctypes.POINTER(ctypes.c_char_p)
            if base in _VOID_POINTEES or base in opaque:
                return ctypes.POINTER(ctypes.c_void_p)
        fail(pos, f"no rule for the type {decl.strip()!r} of {what}")

    def struct_fields(name, body, pos):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.fullmatch(r"(\w+) (.+)", decl)
            if not m or m.group(1) not in _SCALARS:
                fail(pos, f"struct {name}: no rule for the field declaration {decl!r}")
            for declarator in m.group(2).split(","):
                f = re.fullmatch(r"(\w+)((?:\[\w+\])*)", declarator.strip())  # a pointer, a bit-field, an expression as extent: refused
                if not f:
                    fail(pos, f"struct {name}: no rule for the declarator {declarator.strip()!r} in {decl!r}")
                t = _SCALARS[m.group(1)]
                for extent in reversed(re.findall(r"\[(\w+)\]", f.group(2))):
                    if not extent.isdigit() and extent not in constants:
                        fail(pos, f"struct {name}: array extent {extent!r} of {f.group(1)!r} is no integer and no macro defined above it")
                    t = t * (int(extent) if extent.isdigit() else constants[extent])
                fields.append((f.group(1), t))
        return fields

    def parameters(name, params, pos):
        argtypes = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            a = re.fullmatch(r"(.+?[ *])(\w+)", p.strip())
            if not a or a.group(2) in _SCALARS or a.group(2) in ("void", "const"):
                fail(pos, f"{name}: parameter {p.strip()!r} has no name (or is no plain 'type name')")
            argtypes.append(ctype(a.group(1), pos, f"{name}'s parameter {a.group(2)!r}"))
        return argtypes

    end = 0
    for m in re.finditer(r"\s*([^;{}]*(?:\{[^{}]*\}[^;{}]*)*);", text):  # one statement: up to the first ';' outside braces
        if m.start() != end:
            fail(end, "unbalanced braces")
        end, pos = m.end(), m.start(1)
        s = " ".join(m.group(1).split())
        fwd = re.fullmatch(r"typedef struct (\w+) (\w+)", s)
        full = re.fullmatch(r"typedef struct (\w+) ?\{(.*)\} ?(\w+)", s)
        fnptr = re.fullmatch(r"typedef void ?\( ?\* ?(\w+) ?\) ?\(([^()]*)\)", s)
        proto = re.fullmatch(r"(.+?[ *])(\w+) ?\(([^()]*)\)", s)
        if fwd and fwd.group(1) == fwd.group(2):
            opaque.add(fwd.group(1))
        elif full and full.group(1) == full.group(3) and full.group(1) not in structs:
            name = full.group(1)
            cls_name = _CLASS_NAMES.get(name) or "".join(p.capitalize() for p in name.split("_"))
            structs[name] = type(cls_name, (ctypes.Structure,), {"_fields_": struct_fields(name, full.group(2), pos),
                                                                 "__doc__": f"{name} ({os.path.basename(path)})."})
        elif fnptr:
            fn = callbacks.get(fnptr.group(1))
            if fn is None or fn._restype_ is not None or list(fn._argtypes_) != parameters(fnptr.group(1), fnptr.group(2), pos):
                fail(pos, f"function-pointer typedef {fnptr.group(1)!r} has no CFUNCTYPE of these parameters in the binding")
        elif proto and not s.startswith("typedef") and proto.group(2) not in prototypes:
            name = proto.group(2)
            prototypes[name] = (ctype(proto.group(1), pos, f"{name}'s return value", ret=True), parameters(name, proto.group(3), pos))
        else:
            fail(pos, f"no rule for the declaration {s[:100]!r}")
    if text[end:].strip():
        fail(end, f"text outside any declaration: {text[end:].strip()[:60]!r}")
    return constants, structs, prototypes


def _parse_own_header():
    try:
        with open(HEADER_PATH, encoding="utf-8") as f:
            text = f.read()
    except OSError as e:
        raise RuntimeError(f"{HEADER_PATH} not found ({e.strerror}): the binding is derived from the C ABI header, which is looked for at "
                           "../include/hificar.h from the articulatory_amd package (run from the repository tree)") from e
    return parse_header(text, HEADER_PATH)


_CONSTANTS, STRUCTS, PROTOTYPES = _parse_own_header()
# HIFICAR_PREC_F32 -> PREC_F32, HIFICAR_MAX_STAGES -> MAX_STAGES, HIFICAR_E_INVALID -> E_INVALID, ...: every integer macro of the header
CONSTANTS = {k[len("HIFICAR_"):]: v for k, v in _CONSTANTS.items() if k.startswith("HIFICAR_")}
globals().update(CONSTANTS)
# hificar_config -> HificarConfig, hificar_kernel_stat -> HificarKernelStat, ...: every struct of the header
globals().update({cls.__name__: cls for cls in STRUCTS.values()})
# every function the header declares, known without loading the library (tests/test_cabi.py checks the .so exports each one)
SYMBOLS = tuple(PROTOTYPES)

PRECISIONS = {"f32": PREC_F32, "bf16x3": PREC_BF16X3}  # the inference arithmetics (``precision=``)
# ... and the Transformer's training arithmetics (``train_precision=``): bf16x3w = bf16x3 with the one-tap weight gradients in it too
TRAIN_PRECISIONS = dict(PRECISIONS, bf16x3w=PREC_BF16X3W)
# the Transformer's inference arithmetics: bf16x3a is bf16x3 with the attention's products on bf16 MFMAs too
XFMR_PRECISIONS = dict(PRECISIONS, bf16x3a=PREC_BF16X3A)
# the HuBERT encoder's (features.HuBERT): the same three names, defined as for the Transformer
HUBERT_PRECISIONS = dict(PRECISIONS, bf16x3a=PREC_BF16X3A)
# the Transformer's training arithmetics with bf16x3wa: bf16x3w with the attention's query-tiled kernels (forward, backward-q) on bf16 MFMAs too
XFMR_TRAIN_PRECISIONS = dict(TRAIN_PRECISIONS, bf16x3wa=PREC_BF16X3WA)
# ... and with bf16x3wac: bf16x3wa with the weight gradients of the wide k = 3 ResBlock convs on bf16 MFMAs too (what ``train_precision=`` accepted before bf16x3wack)
XFMR_TRAIN_PRECISIONS_ALL = dict(XFMR_TRAIN_PRECISIONS, bf16x3wac=PREC_BF16X3WAC)
# ... and with bf16x3wack: bf16x3wac with the attention's key-tiled backward (dK, dV, the tables' gradient) on bf16 MFMAs too: every value
# ``train_precision=`` accepts (the three mappings above stay as they are: they are what their arithmetics' tests pin)
XFMR_TRAIN_PRECISIONS_K = dict(XFMR_TRAIN_PRECISIONS_ALL, bf16x3wack=PREC_BF16X3WACK)

_lib = None


def load_library():
    """Load libhificar.so (once) and declare every prototype of the header.  Raises RuntimeError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (or `make -C articulatory_amd/csrc`). "
            "There is no CPU fallback for the generator forward pass."
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def profile_rows(lib, engine, capacity):
    """hificar_profile_end on ``engine`` into ``capacity`` rows -> (rows, n): the rows the library filled, as dicts with the fields of
    hificar_kernel_stat (name, launches, total_ms, flops, bytes), and the number n of distinct kernels it reported (n > capacity: rows
    were dropped)."""
    stats = (HificarKernelStat * capacity)()
    n = ctypes.c_int(0)
    check(lib.hificar_profile_end(engine, stats, capacity, ctypes.byref(n)), "hificar_profile_end")
    rows = [dict(name=s.name.decode(), launches=int(s.launches), total_ms=float(s.total_ms), flops=float(s.flops), bytes=float(s.bytes))
            for s in stats[:min(n.value, capacity)]]
    return rows, n.value


def check_interp_factor(interp_factor) -> int:
    """``interp_factor`` of ``forward_lowrate`` as hificar_*_forward_lowrate takes it: an integer in 1 .. 16 (ValueError otherwise, before any
    device work)."""
    import numbers

    if isinstance(interp_factor, bool) or not isinstance(interp_factor, numbers.Integral):
        raise ValueError(f"interp_factor must be an integer in 1 .. {LOWRATE_MAX_FACTOR}, got {interp_factor!r}")
    if not 1 <= int(interp_factor) <= LOWRATE_MAX_FACTOR:
        raise ValueError(f"interp_factor must lie in 1 .. {LOWRATE_MAX_FACTOR}, got {interp_factor}")
    return int(interp_factor)


def check(rc, what):
    if rc != 0:
        msg = load_library().hificar_last_error().decode("utf-8", "replace")
        exc = ValueError if rc == E_INVALID else RuntimeError
        raise exc(f"{what}: {msg} (hificar error {rc})")


def make_config(params: dict, precision: int) -> HificarConfig:
    """generator_params (reference YAML keys) -> hificar_config."""
    cfg = HificarConfig()
    scales = list(params["upsample_scales"])
    ksizes = list(params["upsample_kernel_sizes"])
    rks = list(params["resblock_kernel_sizes"])
    rds = [list(d) for d in params["resblock_dilations"]]
    if len(scales) > MAX_STAGES or len(rks) > MAX_BLOCKS or any(len(d) > MAX_DILATIONS for d in rds):
        raise ValueError("generator is larger than the C ABI's fixed-size config arrays")
    cfg.in_channels = params["in_channels"]
    cfg.out_channels = params["out_channels"]
    cfg.channels = params["channels"]
    cfg.kernel_size = params["kernel_size"]
    cfg.n_stages = len(scales)
    for i, (s, k) in enumerate(zip(scales, ksizes)):
        cfg.upsample_scales[i] = s
        cfg.upsample_kernel_sizes[i] = k
    cfg.n_blocks = len(rks)
    for j, k in enumerate(rks):
        cfg.resblock_kernel_sizes[j] = k
        cfg.n_dilations[j] = len(rds[j])
        for d, v in enumerate(rds[j]):
            cfg.resblock_dilations[j][d] = v
    cfg.use_additional_convs = int(params["use_additional_convs"])
    cfg.bias = int(params["bias"])
    cfg.lrelu_slope = float(params["nonlinear_activation_params"].get("negative_slope", 0.01))
    cfg.use_tanh = int(params["use_tanh"])
    cfg.use_ar = int(params["use_ar"])
    cfg.ar_input = params["ar_input"]
    cfg.ar_hidden = params["ar_hidden"]
    cfg.ar_output = params["ar_output"]
    cfg.precision = precision
    cfg.use_spk_id = int(params.get("use_spk_id", False))
    cfg.num_spk = int(params.get("num_spk") or 0)
    cfg.spk_emb_size = int(params.get("spk_emb_size") or 0)
    cfg.use_ph = int(params.get("use_ph", False))
    cfg.num_ph = int(params.get("num_ph") or 0)
    cfg.ph_emb_size = int(params.get("ph_emb_size") or 0)
    cfg.use_ph_loss = int(params.get("use_ph_loss", False))
    return cfg


# what hificar_gblock_create accepts (csrc/hificar_gblock.hip.inc); GBlockGenerator.__init__ checks the same numbers so that an unsupported
# configuration fails at construction, not at the first forward on the device
GBLOCK_MAX_KERNEL = 11   # odd g_kernel_sizes up to this (the dilation-27 conv's halo against the LDS)
GBLOCK_MAX_SCALE = 64
GBLOCK_MAX_CONV_KERNEL = 16  # input / output conv kernel_size (kMaxTaps)


def check_gblock_params(params: dict):
    """ValueError for a configuration libhificar's GBlock engine rejects (the reference's own limits are checked by the class)."""
    if params["out_channels"] != 1:
        raise ValueError(f"out_channels={params['out_channels']} unsupported (1 only)")
    if params["kernel_size"] > GBLOCK_MAX_CONV_KERNEL:
        raise ValueError(f"kernel_size={params['kernel_size']} > {GBLOCK_MAX_CONV_KERNEL}")
    if params["channels"] // 8 < 1:
        raise ValueError(f"channels={params['channels']} leaves no channels for the last GBlocks")
    for i, (s, k) in enumerate(zip(params["g_scales"], params["g_kernel_sizes"])):
        if k > GBLOCK_MAX_KERNEL:
            raise ValueError(f"g_kernel_sizes[{i}]={k} > {GBLOCK_MAX_KERNEL} (the dilation-27 conv's halo must fit the LDS tiles)")
        if not 1 <= s <= GBLOCK_MAX_SCALE:
            raise ValueError(f"g_scales[{i}]={s} out of range (1 .. {GBLOCK_MAX_SCALE})")
    if params.get("use_ar"):
        if params["ar_input"] < 1 or params["ar_input"] > 1024 or params["ar_hidden"] > 512 or params["ar_output"] > 512:
            raise ValueError("PastFCEncoder: ar_input must be 1 .. 1024, ar_hidden / ar_output <= 512")
        if params["ar_hidden"] % 4 or params["ar_output"] % 4:
            raise ValueError("PastFCEncoder hidden / output dims must be multiples of 4")
    if params.get("use_spk_id") and (not params.get("num_spk") or (params.get("spk_emb_size") or 0) < 1 or params["in_channels"] > 1024):
        raise ValueError("use_spk_id needs num_spk and spk_emb_size (and in_channels <= 1024)")


def make_gblock_config(params: dict, precision: int) -> HificarGBlockConfig:
    """generator_params of a GBlockGenerator (reference keyword names) -> hificar_gblock_config."""
    cfg = HificarGBlockConfig()
    scales, ksizes = list(params["g_scales"]), list(params["g_kernel_sizes"])
    if len(scales) > MAX_GBLOCKS:
        raise ValueError(f"{len(scales)} GBlocks: the reference's channel plan has {MAX_GBLOCKS} entries (gblock_gen.py:63-64)")
    cfg.in_channels = params["in_channels"]
    cfg.out_channels = params["out_channels"]
    cfg.channels = params["channels"]
    cfg.kernel_size = params["kernel_size"]
    cfg.n_blocks = len(scales)
    for i, (s, k) in enumerate(zip(scales, ksizes)):
        cfg.g_scales[i] = s
        cfg.g_kernel_sizes[i] = k
    cfg.use_tanh = int(params["use_tanh"])
    cfg.use_ar = int(params["use_ar"])
    cfg.ar_input = params["ar_input"]
    cfg.ar_hidden = params["ar_hidden"]
    cfg.ar_output = params["ar_output"]
    cfg.use_spk_id = int(params.get("use_spk_id", False))
    cfg.num_spk = int(params.get("num_spk") or 0)
    cfg.spk_emb_size = int(params.get("spk_emb_size") or 0)
    cfg.precision = precision
    return cfg


# what hificar_bigru_create accepts (csrc/hificar_bigru.hip.inc; HIFICAR_BIGRU_MAX_* of include/hificar.h); BiGRU.__init__ checks the same
# numbers so that an unsupported configuration fails at construction, not at the first forward on the device
# (BIGRU_MAX_HIDDEN: one workgroup holds one direction's W_hh in registers + LDS + a streamed remainder; BIGRU_MAX_OUT: fc2's rows in the head
# kernel's LDS)


def check_bigru_params(params: dict):
    """ValueError for a BiGRU configuration libhificar's engine rejects."""
    h = params["hidden_size"]
    if not 1 <= params["in_channels"] <= BIGRU_MAX_IN:
        raise ValueError(f"in_channels={params['in_channels']} out of range (1 .. {BIGRU_MAX_IN})")
    if h < 64 or h > BIGRU_MAX_HIDDEN or h % 64:
        raise ValueError(f"hidden_size={h} unsupported (multiples of 64 up to {BIGRU_MAX_HIDDEN}: one workgroup holds a direction's W_hh)")
    if not 1 <= params["out_channels"] <= BIGRU_MAX_OUT:
        raise ValueError(f"out_channels={params['out_channels']} out of range (1 .. {BIGRU_MAX_OUT})")


def make_bigru_config(params: dict) -> HificarBigruConfig:
    """BiGRU keyword arguments (reference names) -> hificar_bigru_config."""
    cfg = HificarBigruConfig()
    cfg.in_channels = params["in_channels"]
    cfg.hidden_size = params["hidden_size"]
    cfg.out_channels = params["out_channels"]
    cfg.use_tanh = int(params["use_tanh"])
    return cfg


# what hificar_xfmr_create accepts (csrc/hificar_xfmr.hip.inc; HIFICAR_XFMR_MAX_* of include/hificar.h); Transformer.__init__ checks the same
# numbers so that an unsupported configuration fails at construction, before any device work
# (XFMR_MAX_OUT: w_out's rows share the feed-forward buffer; XFMR_MAX_HIDDEN: head size hidden_dim / 8 up to 128, the attention kernel's
# instantiations)
XFMR_HEADS = 8           # nhead, dim_feedforward, relative_positional_distance: the reference constructor's constants (transformer.py:43)
XFMR_FF = 3072
XFMR_REL = 100


def check_xfmr_params(params: dict):
    """ValueError for a Transformer configuration libhificar's engine rejects."""
    f = params["hidden_dim"]
    if not 1 <= params["in_channels"] <= XFMR_MAX_IN:
        raise ValueError(f"in_channels={params['in_channels']} out of range (1 .. {XFMR_MAX_IN})")
    if not 1 <= params["out_channels"] <= XFMR_MAX_OUT:
        raise ValueError(f"out_channels={params['out_channels']} out of range (1 .. {XFMR_MAX_OUT})")
    if not 1 <= params["elayers"] <= XFMR_MAX_LAYERS:
        raise ValueError(f"elayers={params['elayers']} out of range (1 .. {XFMR_MAX_LAYERS})")
    if f < 128 or f > XFMR_MAX_HIDDEN or f % 128:
        raise ValueError(f"hidden_dim={f} unsupported (multiples of 128 up to {XFMR_MAX_HIDDEN}: the attention kernel is built for head sizes 16 .. 128)")


def make_xfmr_config(params: dict) -> HificarXfmrConfig:
    """Transformer keyword arguments (reference names) -> hificar_xfmr_config."""
    cfg = HificarXfmrConfig()
    cfg.in_channels = params["in_channels"]
    cfg.out_channels = params["out_channels"]
    cfg.elayers = params["elayers"]
    cfg.hidden_dim = params["hidden_dim"]
    return cfg


# what hificar_hubert_create accepts (csrc/hificar_hubert.hip.inc; HIFICAR_HUBERT_* of include/hificar.h); features.HuBERT checks the same
# numbers, and everything about the architecture that is not built, at construction: from a configuration alone, before any device work
HUBERT_CONV_KERNEL = (10, 3, 3, 3, 3, 2, 2)
HUBERT_CONV_STRIDE = (5, 2, 2, 2, 2, 2, 2)
HUBERT_POS_TAPS = 128
HUBERT_POS_GROUPS = 16
HUBERT_HIDDEN_SIZES = (128, 256, 512, 768, 1024)  # 16 positional groups of 8, 16, 32, 48 or 64 channels: hubert_posconv_kernel's instantiations
# the library's defaults for the keys a "large" config.json may leave out (transformers' HubertConfig), with the large family's switches on
HUBERT_DEFAULTS = dict(conv_dim=(512,) * 7, conv_kernel=HUBERT_CONV_KERNEL, conv_stride=HUBERT_CONV_STRIDE, hidden_size=1024, num_hidden_layers=24,
                       num_attention_heads=16, intermediate_size=4096, conv_bias=True, feat_extract_norm="layer", do_stable_layer_norm=True,
                       feat_proj_layer_norm=True, layer_norm_eps=1e-5, num_conv_pos_embeddings=HUBERT_POS_TAPS,
                       num_conv_pos_embedding_groups=HUBERT_POS_GROUPS, hidden_act="gelu", feat_extract_activation="gelu", mask_time_prob=0.05,
                       mask_feature_prob=0.0)


def check_hubert_config(config: dict) -> dict:
    """A ``config.json`` mapping of a HuBERT model -> the same with the defaults filled in.  NotImplementedError for an architecture that is
    not built (group-norm extractors, post-LN encoders, WavLM's gated relative position bias, adapters, other activations or conv plans),
    ValueError for widths outside hificar_hubert_create's limits."""
    c = dict(HUBERT_DEFAULTS)
    c.update(config)
    if str(c.get("model_type", "hubert")).lower() != "hubert" or any(k in c for k in ("num_buckets", "max_bucket_distance")):
        raise NotImplementedError(f"HuBERT: model_type {c.get('model_type')!r}: WavLM's gated relative position bias is not built (HuBERT only)")
    if c["feat_extract_norm"] != "layer":
        raise NotImplementedError(f"HuBERT: feat_extract_norm={c['feat_extract_norm']!r}: group-norm extractors (HuBERT-base) are not built; "
                                  "only the large family's layer-norm extractor is")
    if not c["do_stable_layer_norm"]:
        raise NotImplementedError("HuBERT: do_stable_layer_norm=False: post-LN encoders (HuBERT-base) are not built")
    if not c["feat_proj_layer_norm"]:
        raise NotImplementedError("HuBERT: feat_proj_layer_norm=False is not built")
    if tuple(c["conv_kernel"]) != HUBERT_CONV_KERNEL or tuple(c["conv_stride"]) != HUBERT_CONV_STRIDE:
        raise NotImplementedError(f"HuBERT: conv_kernel / conv_stride {tuple(c['conv_kernel'])} / {tuple(c['conv_stride'])}: only "
                                  f"{HUBERT_CONV_KERNEL} / {HUBERT_CONV_STRIDE} is built")
    if c["hidden_act"] != "gelu" or c["feat_extract_activation"] != "gelu":
        raise NotImplementedError(f"HuBERT: activations {c['hidden_act']!r} / {c['feat_extract_activation']!r}: only 'gelu' (erf form) is built")
    if c["num_conv_pos_embeddings"] != HUBERT_POS_TAPS or c["num_conv_pos_embedding_groups"] != HUBERT_POS_GROUPS or c.get("conv_pos_batch_norm"):
        raise NotImplementedError(f"HuBERT: only the weight-normed positional conv of {HUBERT_POS_TAPS} taps in {HUBERT_POS_GROUPS} groups is built")
    if c.get("adapter_attn_dim") is not None:
        raise NotImplementedError("HuBERT: attention adapters are not built")
    dims = tuple(c["conv_dim"])
    if len(dims) != len(HUBERT_CONV_KERNEL) or len(set(dims)) != 1:
        raise NotImplementedError(f"HuBERT: conv_dim={dims}: seven extractor layers of one width are built")
    if dims[0] < 32 or dims[0] > HUBERT_MAX_CONV or dims[0] % 32:
        raise ValueError(f"HuBERT: conv_dim={dims[0]} unsupported (multiples of 32 up to {HUBERT_MAX_CONV})")
    if c["hidden_size"] not in HUBERT_HIDDEN_SIZES:
        raise ValueError(f"HuBERT: hidden_size={c['hidden_size']} unsupported ({HUBERT_HIDDEN_SIZES}: 16 positional groups of 8 .. 64 channels)")
    if c["num_attention_heads"] * HUBERT_HEAD_DIM != c["hidden_size"]:
        raise ValueError(f"HuBERT: {c['num_attention_heads']} heads of hidden_size={c['hidden_size']}: head size {HUBERT_HEAD_DIM} is required "
                         "(the attention kernel's one instantiation)")
    if c["intermediate_size"] < 32 or c["intermediate_size"] > HUBERT_MAX_FFN or c["intermediate_size"] % 32:
        raise ValueError(f"HuBERT: intermediate_size={c['intermediate_size']} unsupported (multiples of 32 up to {HUBERT_MAX_FFN})")
    if not 1 <= c["num_hidden_layers"] <= HUBERT_MAX_LAYERS:
        raise ValueError(f"HuBERT: num_hidden_layers={c['num_hidden_layers']} out of range (1 .. {HUBERT_MAX_LAYERS})")
    return c


# WavLM (features.WavLM): HuBERT-large's encoder with the gated relative position bias; the published wavlm-large's table
WAVLM_DEFAULTS = dict(num_buckets=320, max_bucket_distance=800)
# the encoder's arithmetics under the bias: the bf16 attention kernel (bf16x3a) has no bias term
WAVLM_PRECISIONS = dict(PRECISIONS)


def check_wavlm_config(config: dict) -> dict:
    """A ``config.json`` mapping of a WavLM model -> the same with the defaults filled in (the large model's; ``num_buckets`` 320,
    ``max_bucket_distance`` 800).  Everything check_hubert_config refuses stays refused, under WavLM's name: group-norm extractors and post-LN
    encoders (wavlm-base, wavlm-base-plus), adapters, head sizes other than 64."""
    c = dict(config)
    model_type = str(c.pop("model_type", "wavlm")).lower()
    if model_type != "wavlm":
        raise NotImplementedError(f"WavLM: model_type {model_type!r} (features.HuBERT reads HuBERT configurations)")
    rel = {k: c.pop(k, v) for k, v in WAVLM_DEFAULTS.items()}
    try:
        c = check_hubert_config(c)
    except (NotImplementedError, ValueError) as e:
        raise type(e)(str(e).replace("HuBERT", "WavLM")) from None
    nb, md = rel["num_buckets"], rel["max_bucket_distance"]
    for k, v in rel.items():
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"WavLM: {k} must be an integer, got {v!r}")
    if nb < 4 or nb % 2 or nb > HUBERT_MAX_BUCKETS:
        raise ValueError(f"WavLM: num_buckets={nb} unsupported (even, 4 .. {HUBERT_MAX_BUCKETS})")
    if not nb // 4 < md <= HUBERT_MAX_DISTANCE:
        raise ValueError(f"WavLM: max_bucket_distance={md} unsupported (above num_buckets // 4 = {nb // 4}, the last exact bucket, up to "
                         f"{HUBERT_MAX_DISTANCE})")
    c.update(rel, model_type="wavlm")
    return c


def wavlm_bucket_of_distance(num_buckets: int, max_distance: int):
    """int32 tensor of 2 max_distance + 1 entries: entry d + max_distance is the bucket of the relative position d = key - query, for d in
    -max_distance .. max_distance, by the very float32 operations of the ``transformers`` library's ``WavLMAttention._relative_positions_bucket``
    (a one-ulp difference of the logarithm at a bucket's edge would pick the neighbouring embedding row).  From |d| = max_distance on the
    bucket is the side's last, so hificar_hubert_set_rel_bias's clamp of d into this range is exact.  The one place the map is computed."""
    import math

    import torch

    relative_positions = torch.arange(-max_distance, max_distance + 1, dtype=torch.long)
    nb = num_buckets // 2
    relative_buckets = (relative_positions > 0).to(torch.long) * nb
    relative_positions = torch.abs(relative_positions)
    max_exact = nb // 2
    is_small = relative_positions < max_exact
    if_large = torch.log(relative_positions.float() / max_exact)
    if_large = if_large / math.log(max_distance / max_exact)
    if_large = if_large * (nb - max_exact)
    if_large = (max_exact + if_large).to(torch.long)
    if_large = torch.min(if_large, torch.full_like(if_large, nb - 1))
    relative_buckets += torch.where(is_small, relative_positions, if_large)
    return relative_buckets.to(torch.int32).contiguous()


def make_hubert_config(config: dict, normalize: bool, norm_eps: float) -> HificarHubertConfig:
    """A checked HuBERT configuration (check_hubert_config) -> hificar_hubert_config."""
    cfg = HificarHubertConfig()
    cfg.conv_dim = config["conv_dim"][0]
    cfg.hidden_size = config["hidden_size"]
    cfg.num_hidden_layers = config["num_hidden_layers"]
    cfg.num_attention_heads = config["num_attention_heads"]
    cfg.intermediate_size = config["intermediate_size"]
    cfg.conv_bias = int(bool(config["conv_bias"]))
    cfg.normalize = int(bool(normalize))
    cfg.layer_norm_eps = float(config["layer_norm_eps"])
    cfg.norm_eps = float(norm_eps)
    return cfg


def hubert_frames(length) -> int:
    """50-Hz frames of an utterance of ``length`` samples (hificar_hubert_frames): (length - 400) // 320 + 1; ValueError under 400 samples."""
    if int(length) < HUBERT_MIN_SAMPLES:
        raise ValueError(f"HuBERT: {int(length)} samples: an utterance under {HUBERT_MIN_SAMPLES} samples has no frame")
    return (int(length) - 400) // 320 + 1
