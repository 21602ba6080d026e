// The Transformer feature model (articulatory/models/transformer.py:21-105): features (B, in_channels, T) -> features (B, out_channels, T), eval mode.
//   rows        (B, C, T) -> channels-last rows, and back at the end                       xfmr_rows_kernel / xfmr_out_kernel
//   conv_blocks three ResBlocks (pytorch_layers.py:94-125), the eval-mode BatchNorm1ds folded into their convs: conv1 writes its ReLU'd copy,
//               conv2 takes the block input (block 0: the folded 1 x 1 residual_path) as its fp32 residual and writes the ReLU'd sum      conv engine
//   w_raw_in    Linear(F, F)                                                                conv engine, one-tap launch
//   per layer   q, k, v as ONE GEMM (N = 3 F, no bias)                                      conv engine
//               banded relative-position attention -> rows [head][d]                        xfmr_attn_kernel
//               w_o (no bias) + the layer input as residual, LayerNorm                      conv engine, xfmr_ln_kernel
//               linear1 (ReLU'd copy), linear2 + residual, LayerNorm                        conv engine, xfmr_ln_kernel
//   w_out       Linear(F, out)                                                              conv engine
// Every launch is per sequence (nseq = B, rows = T) under the ragged context: rows at or past a sequence's length read as zero padding and
// are never written, so the k = 3 convs see each utterance's own end.  Exact fp32, split-K off: one accumulation order whatever the batch.
// Workspace: the input rows, three row buffers [B T][F] that rotate, and one wide buffer [B T][3072] (q | k | v, then the feed-forward's
// hidden rows, then w_out's rows).
//
// bf16x3 (hificar_xfmr_set_precision, eval only): every GEMM above runs in the engine's bf16x3 kernels, whose input is "split rows"
// [hi: C bf16 | lo: C bf16] (4 C bytes per row, as fp32 rows) written by the producer: the engine's own output pass (ys), xfmr_rows_split_kernel,
// xfmr_ln_kernel<true>, xfmr_attn_kernel<D, false, true>.  Everything else — attention, LayerNorm, bias and residual additions, the residual
// stream — is fp32 as above.  Five row buffers instead of three: a GEMM's fp32 residual and the next GEMM's split input exist side by side.
//
// bf16x3a (HIFICAR_PREC_BF16X3A, eval only): the bf16x3 forward with the attention's three products on bf16 MFMAs too
// (hificar_xfmr_attn16.hip.h).  The q | k | v GEMM writes split rows only ([hi: 3 F bf16 | lo: 3 F bf16], the bytes of the fp32 row), and
// finalize splits each layer's position tables once.  The conv engine sees a bf16x3 handle.

struct XfmrEncLayer {
    ConvLayer qkv, wo, l1, l2;
    float* d_emb = nullptr;                 // [8][199][d]
    uint16_t* d_emb16 = nullptr;            // bf16x3a: [hi, lo][8][208][d] bf16, rows 199 .. 207 zeros
    float* d_ln[4] = {nullptr, nullptr, nullptr, nullptr};  // norm1.weight, norm1.bias, norm2.weight, norm2.bias
};

struct XfmrTrain;  // hificar_xfmr_train.hip.inc

struct hificar_xfmr {
    hificar_xfmr_config cfg;
    hificar_engine eng;
    WeightIntake weights;
    ConvLayer c1[3], c2[3], rp, w_in, w_out;
    std::vector<XfmrEncLayer> enc;  // sized once, in hificar_xfmr_create (launch plans are keyed by the layers' addresses)
    int cin_pad = 0;
    int precision = HIFICAR_PREC_F32;  // hificar_xfmr_set_precision: which fragments finalize packs and which kernels the forward launches
    // hificar_xfmr_set_train_precision: the arithmetic of the training step's forward and data-gradient GEMMs (an f32 handle only; the eval
    // forward goes by `precision` alone)
    int train_precision = HIFICAR_PREC_F32;
    bool finalized = false;
    TapTable taps;
    XfmrTrain* train = nullptr;  // built by the first training entry point
    int train_failed = HIFICAR_OK;
};

static void xfmr_train_free(hificar_xfmr* g);

// The arithmetics, one row per HIFICAR_PREC_* value: which setter takes it and what it switches on.
//   x3  the GEMMs run in the engine's bf16x3 kernels        w  training: the one-tap GEMM-form weight gradients on bf16 MFMAs
//   a   the attention's query-tiled kernels on bf16 MFMAs    c  training: the wide k = 3 convs' weight gradients on bf16 MFMAs
//   k   training: the attention's key-tiled backward on bf16 MFMAs
struct XfmrArith {
    int value;
    const char* name;
    bool eval, train;  // hificar_xfmr_set_precision, hificar_xfmr_set_train_precision
    bool x3, w, a, c, k;
};
static const XfmrArith kXfmrArith[] = {
    {HIFICAR_PREC_F32, "f32", true, true, false, false, false, false, false},
    {HIFICAR_PREC_BF16X3, "bf16x3", true, true, true, false, false, false, false},
    {HIFICAR_PREC_BF16X3W, "bf16x3w", false, true, true, true, false, false, false},
    {HIFICAR_PREC_BF16X3A, "bf16x3a", true, false, true, false, true, false, false},
    {HIFICAR_PREC_BF16X3WA, "bf16x3wa", false, true, true, true, true, false, false},
    {HIFICAR_PREC_BF16X3WAC, "bf16x3wac", false, true, true, true, true, true, false},
    {HIFICAR_PREC_BF16X3WACK, "bf16x3wack", false, true, true, true, true, true, true},
};
// null: no such arithmetic
static const XfmrArith* xfmr_arith_find(int p) {
    for (const XfmrArith& a : kXfmrArith)
        if (a.value == p) return &a;
    return nullptr;
}
// (of a handle's own field: the setters let nothing else in)
static const XfmrArith& xfmr_arith(int p) {
    const XfmrArith* a = xfmr_arith_find(p);
    return a ? *a : kXfmrArith[0];
}
static const char* xfmr_precision_name(int p) { return xfmr_arith(p).name; }

// the handle's GEMMs run in the engine's bf16x3 kernels (bf16x3 and bf16x3a differ in the attention alone)
static bool xfmr_x3(const hificar_xfmr* g) { return xfmr_arith(g->precision).x3; }

static bool xfmr_head_dim_built(int d) { return d >= 16 && d <= 128 && d % 16 == 0; }

// The one head-size dispatch: fn(std::integral_constant<int, D>) for the instantiation D = d.
template <class Fn>
static hipError_t xfmr_by_d(int d, Fn&& fn) {
    switch (d) {
        case 16: return fn(std::integral_constant<int, 16>());
        case 32: return fn(std::integral_constant<int, 32>());
        case 48: return fn(std::integral_constant<int, 48>());
        case 64: return fn(std::integral_constant<int, 64>());
        case 80: return fn(std::integral_constant<int, 80>());
        case 96: return fn(std::integral_constant<int, 96>());
        case 112: return fn(std::integral_constant<int, 112>());
        case 128: return fn(std::integral_constant<int, 128>());
    }
    return hipErrorInvalidValue;
}
// ... and for every head size in turn, until one fails
template <class Fn>
static hipError_t xfmr_for_every_d(Fn&& fn) {
    for (int d = 16; xfmr_head_dim_built(d); d += 16) {
        const hipError_t e = xfmr_by_d(d, fn);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// one 256-thread launch of an attention kernel
template <class... P, class... A>
static hipError_t xfmr_launch(void (*kernel)(P...), dim3 grid, size_t lds_bytes, hipStream_t stream, const A&... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds_bytes, stream, args...);
    return hipGetLastError();
}

static XfmrTab16 xfmr_tab16(const uint16_t* d_emb16, int d) { return {d_emb16, d_emb16 + (size_t)kXfmrHeads * kXfmrTabPad * d}; }

static int xfmr_plan(ConvLayer& L, const std::string& name, int cin, int cin_pad, int cout, int K) {
    L.name = name;
    L.cin = cin;
    L.cin_pad = cin_pad;
    L.cout = cout;
    L.K = K;
    L.padding = K / 2;
    return plan_layer(L);
}

extern "C" int hificar_xfmr_create(const hificar_xfmr_config* cfg, hificar_xfmr** out) {
    if (!cfg || !out) return fail(HIFICAR_E_INVALID, "hificar_xfmr_create: null argument");
    const hificar_xfmr_config& c = *cfg;
    if (c.in_channels < 1 || c.in_channels > HIFICAR_XFMR_MAX_IN)
        return fail(HIFICAR_E_INVALID, "Transformer: in_channels=%d out of range (1 .. %d)", c.in_channels, HIFICAR_XFMR_MAX_IN);
    if (c.out_channels < 1 || c.out_channels > HIFICAR_XFMR_MAX_OUT)
        return fail(HIFICAR_E_INVALID, "Transformer: out_channels=%d out of range (1 .. %d)", c.out_channels, HIFICAR_XFMR_MAX_OUT);
    if (c.elayers < 1 || c.elayers > HIFICAR_XFMR_MAX_LAYERS)
        return fail(HIFICAR_E_INVALID, "Transformer: elayers=%d out of range (1 .. %d)", c.elayers, HIFICAR_XFMR_MAX_LAYERS);
    if (c.hidden_dim < 128 || c.hidden_dim > HIFICAR_XFMR_MAX_HIDDEN || c.hidden_dim % 128 != 0 || !xfmr_head_dim_built(c.hidden_dim / kXfmrHeads))
        return fail(HIFICAR_E_INVALID, "Transformer: hidden_dim=%d unsupported (multiples of 128 up to %d: the attention kernel is built for head sizes 16 .. 128)",
                    c.hidden_dim, HIFICAR_XFMR_MAX_HIDDEN);
    static_assert(HIFICAR_XFMR_MAX_OUT <= kXfmrFF, "w_out's rows share the feed-forward buffer");
    hificar_xfmr* g = new hificar_xfmr();
    g->cfg = c;
    const int64_t F = c.hidden_dim, C = c.in_channels, O = c.out_channels, d = F / kXfmrHeads;
    g->cin_pad = round_up(c.in_channels, 32);
    for (int i = 0; i < 3; ++i) {
        const std::string b = "conv_blocks." + std::to_string(i) + ".";
        g->weights.expected[b + "conv1.weight"] = {F, i == 0 ? C : F, 3};
        g->weights.expected[b + "conv2.weight"] = {F, F, 3};
        for (const char* m : {"conv1", "conv2", "bn1", "bn2"}) g->weights.expected[b + m + ".bias"] = {F};
        for (const char* m : {"bn1", "bn2"})
            for (const char* t : {".weight", ".running_mean", ".running_var"}) g->weights.expected[b + m + t] = {F};
        if (i == 0 && C != F) {  // (pytorch_layers.py:108-112: the 1 x 1 path exists when the block changes the width)
            g->weights.expected[b + "residual_path.weight"] = {F, C, 1};
            g->weights.expected[b + "residual_path.bias"] = {F};
            for (const char* t : {".weight", ".bias", ".running_mean", ".running_var"}) g->weights.expected[b + "res_norm" + t] = {F};
        }
    }
    g->weights.expected["w_raw_in.weight"] = {F, F};
    g->weights.expected["w_raw_in.bias"] = {F};
    for (int l = 0; l < c.elayers; ++l) {
        const std::string b = "transformer.layers." + std::to_string(l) + ".";
        for (const char* w : {"w_q", "w_k", "w_v"}) g->weights.expected[b + "self_attn." + w] = {kXfmrHeads, F, d};
        g->weights.expected[b + "self_attn.w_o"] = {kXfmrHeads, d, F};
        g->weights.expected[b + "self_attn.relative_positional.embeddings"] = {kXfmrHeads, kXfmrTab, d, 1};
        g->weights.expected[b + "linear1.weight"] = {kXfmrFF, F};
        g->weights.expected[b + "linear1.bias"] = {kXfmrFF};
        g->weights.expected[b + "linear2.weight"] = {F, kXfmrFF};
        g->weights.expected[b + "linear2.bias"] = {F};
        for (const char* n : {"norm1", "norm2"})
            for (const char* t : {".weight", ".bias"}) g->weights.expected[b + n + t] = {F};
    }
    g->weights.expected["w_out.weight"] = {O, F};
    g->weights.expected["w_out.bias"] = {O};
    g->enc.resize((size_t)c.elayers);
    const int Fi = c.hidden_dim;
    int rc = HIFICAR_OK;
    for (int i = 0; i < 3 && rc == HIFICAR_OK; ++i) {
        const std::string b = "conv_blocks." + std::to_string(i);
        rc = xfmr_plan(g->c1[i], b + ".conv1#bn1", i == 0 ? c.in_channels : Fi, i == 0 ? g->cin_pad : Fi, Fi, 3);
        if (rc == HIFICAR_OK) rc = xfmr_plan(g->c2[i], b + ".conv2#bn2", Fi, Fi, Fi, 3);
    }
    if (rc == HIFICAR_OK && c.in_channels != Fi) rc = xfmr_plan(g->rp, "conv_blocks.0.residual_path#res_norm", c.in_channels, g->cin_pad, Fi, 1);
    if (rc == HIFICAR_OK) rc = xfmr_plan(g->w_in, "w_raw_in", Fi, Fi, Fi, 1);
    for (int l = 0; l < c.elayers && rc == HIFICAR_OK; ++l) {
        const std::string b = "transformer.layers." + std::to_string(l);
        XfmrEncLayer& E = g->enc[(size_t)l];
        rc = xfmr_plan(E.qkv, b + ".self_attn#qkv", Fi, Fi, 3 * Fi, 1);
        if (rc == HIFICAR_OK) rc = xfmr_plan(E.wo, b + ".self_attn.w_o", Fi, Fi, Fi, 1);
        if (rc == HIFICAR_OK) rc = xfmr_plan(E.l1, b + ".linear1", Fi, Fi, kXfmrFF, 1);
        if (rc == HIFICAR_OK) rc = xfmr_plan(E.l2, b + ".linear2", kXfmrFF, kXfmrFF, Fi, 1);
    }
    if (rc == HIFICAR_OK) rc = xfmr_plan(g->w_out, "w_out", Fi, Fi, c.out_channels, 1);
    if (rc != HIFICAR_OK) {
        delete g;
        return rc;
    }
    *out = g;
    return HIFICAR_OK;
}

extern "C" void hificar_xfmr_destroy(hificar_xfmr* g) {
    if (!g) return;
    xfmr_train_free(g);
    engine_close(&g->eng);
    delete g;
}

extern "C" hificar_engine* hificar_xfmr_engine(hificar_xfmr* g) { return g ? &g->eng : nullptr; }

extern "C" int hificar_xfmr_set_weight(hificar_xfmr* g, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!g || !name || !data || !shape) return fail(HIFICAR_E_INVALID, "hificar_xfmr_set_weight: null argument");
    if (g->finalized) return fail(HIFICAR_E_STATE, "hificar_xfmr_set_weight(%s) after hificar_xfmr_finalize", name);
    return g->weights.set(name, data, shape, ndim);
}

// bias and weight fragments of one layer, in the engine's arithmetic only (h->precision is set before the first pack): one resident copy
static int xfmr_pack(hificar_engine* h, ConvLayer& L, const HostTensor& W, const std::vector<float>* bias) {
    std::vector<float> b((size_t)L.cout_total, 0.f);
    if (bias) std::copy(bias->begin(), bias->begin() + L.cout, b.begin());
    const int rc = upload(h, b, &L.d_bias);
    if (rc != HIFICAR_OK) return rc;
    if (h->precision == HIFICAR_PREC_BF16X3) return pack_w16(h, L, W, L.chunk16, &L.d_w16);
    return pack_w32(h, L, W, L.chunk16, &L.d_w32);
}

extern "C" int hificar_xfmr_set_precision(hificar_xfmr* g, int precision) {
    if (!g) return fail(HIFICAR_E_INVALID, "hificar_xfmr_set_precision: null handle");
    const XfmrArith* a = xfmr_arith_find(precision);
    if (!a || !a->eval) return fail(HIFICAR_E_INVALID, "unknown precision %d", precision);
    if (g->finalized)
        return fail(HIFICAR_E_STATE, "hificar_xfmr_set_precision after hificar_xfmr_finalize: the weights are packed for %s only; make a new handle",
                    xfmr_precision_name(g->precision));
    g->precision = precision;
    return HIFICAR_OK;
}

// Conv1d followed by an eval-mode BatchNorm1d as one conv: y = (W x + b - mean) * gamma / sqrt(var + 1e-5) + beta, folded in double
static int xfmr_pack_folded(hificar_xfmr* g, ConvLayer& L, const std::string& conv, const std::string& bn) {
    const HostTensor& W = g->weights.at(conv + ".weight");
    const std::vector<float>&b = g->weights.data(conv + ".bias"), &gm = g->weights.data(bn + ".weight"), &bt = g->weights.data(bn + ".bias"),
                     &mu = g->weights.data(bn + ".running_mean"), &var = g->weights.data(bn + ".running_var");
    HostTensor Wf;
    Wf.shape = W.shape;
    Wf.data.resize(W.data.size());
    std::vector<float> bf((size_t)L.cout);
    const size_t per = (size_t)L.cin * L.K;
    for (int o = 0; o < L.cout; ++o) {
        const double s = (double)gm[o] / std::sqrt((double)var[o] + 1e-5);
        for (size_t k = 0; k < per; ++k) Wf.data[o * per + k] = (float)((double)W.data[o * per + k] * s);
        bf[o] = (float)(((double)b[o] - (double)mu[o]) * s + (double)bt[o]);
    }
    return xfmr_pack(&g->eng, L, Wf, &bf);
}

template <int D>
static hipError_t xfmr_attn_attr() {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&xfmr_attn_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)XfmrAttnLds<D>::bytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&xfmr_attn_kernel<D, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)XfmrAttnLds<D>::bytes);
}

extern "C" int hificar_xfmr_finalize(hificar_xfmr* g) {
    if (!g) return fail(HIFICAR_E_INVALID, "hificar_xfmr_finalize: null handle");
    if (g->finalized) return HIFICAR_OK;
    if (const int missing = g->weights.check_complete()) return missing;
    hificar_engine* h = &g->eng;
    const int F = g->cfg.hidden_dim, d = F / kXfmrHeads;
    int rc;
    h->precision = xfmr_x3(g) ? HIFICAR_PREC_BF16X3 : HIFICAR_PREC_F32;  // (xfmr_pack goes by it)
    for (int i = 0; i < 3; ++i) {
        const std::string b = "conv_blocks." + std::to_string(i) + ".";
        if ((rc = xfmr_pack_folded(g, g->c1[i], b + "conv1", b + "bn1")) != HIFICAR_OK) return rc;
        if ((rc = xfmr_pack_folded(g, g->c2[i], b + "conv2", b + "bn2")) != HIFICAR_OK) return rc;
    }
    if (g->rp.cout && (rc = xfmr_pack_folded(g, g->rp, "conv_blocks.0.residual_path", "conv_blocks.0.res_norm")) != HIFICAR_OK) return rc;
    if ((rc = pack_linear(h, g->w_in, g->weights, "w_raw_in")) != HIFICAR_OK) return rc;
    if ((rc = pack_linear(h, g->w_out, g->weights, "w_out")) != HIFICAR_OK) return rc;
    for (int l = 0; l < g->cfg.elayers; ++l) {
        const std::string b = "transformer.layers." + std::to_string(l) + ".";
        XfmrEncLayer& E = g->enc[(size_t)l];
        {   // q = einsum('tbf,hfa->bhta', x, w_q) (pytorch_layers.py:213-215): row (s 8 + h) d + a of the GEMM's weight is w_s[h, :, a]
            HostTensor W;
            W.shape = {3 * F, F, 1};
            W.data.resize((size_t)3 * F * F);
            int s = 0;
            for (const char* w : {"w_q", "w_k", "w_v"}) {
                const std::vector<float>& src = g->weights.data(b + "self_attn." + w);
                for (int hh = 0; hh < kXfmrHeads; ++hh)
                    for (int f = 0; f < F; ++f)
                        for (int a = 0; a < d; ++a) W.data[((size_t)(s * kXfmrHeads + hh) * d + a) * F + f] = src[((size_t)hh * F + f) * d + a];
                ++s;
            }
            if ((rc = xfmr_pack(h, E.qkv, W, nullptr)) != HIFICAR_OK) return rc;
        }
        {   // out = einsum('bhta,haf->tbf', o, w_o) (:228): row f of the GEMM's weight is w_o[:, :, f] over (h, a)
            const std::vector<float>& src = g->weights.data(b + "self_attn.w_o");
            HostTensor W;
            W.shape = {F, F, 1};
            W.data.resize((size_t)F * F);
            for (int k = 0; k < F; ++k)
                for (int f = 0; f < F; ++f) W.data[(size_t)f * F + k] = src[(size_t)k * F + f];
            if ((rc = xfmr_pack(h, E.wo, W, nullptr)) != HIFICAR_OK) return rc;
        }
        if ((rc = pack_linear(h, E.l1, g->weights, b + "linear1")) != HIFICAR_OK) return rc;
        if ((rc = pack_linear(h, E.l2, g->weights, b + "linear2")) != HIFICAR_OK) return rc;
        if ((rc = upload(h, g->weights.data(b + "self_attn.relative_positional.embeddings"), &E.d_emb)) != HIFICAR_OK) return rc;
        if (xfmr_arith(g->precision).a) {  // the tables as the attention's MFMA operand: split once, padded to whole 16-row tiles
            const std::vector<float>& src = g->weights.data(b + "self_attn.relative_positional.embeddings");
            const size_t half = (size_t)kXfmrHeads * kXfmrTabPad * d;
            std::vector<uint16_t> t16(2 * half, 0);
            for (int hh = 0; hh < kXfmrHeads; ++hh)
                for (int r = 0; r < kXfmrTab; ++r)
                    for (int a = 0; a < d; ++a) {
                        const float v = src[((size_t)hh * kXfmrTab + r) * d + a];
                        const uint16_t vh = f32_to_bf16(v);
                        t16[((size_t)hh * kXfmrTabPad + r) * d + a] = vh;
                        t16[half + ((size_t)hh * kXfmrTabPad + r) * d + a] = f32_to_bf16(v - bf16_to_f32(vh));
                    }
            void* dp = nullptr;
            HIP_TRY(hipMalloc(&dp, t16.size() * sizeof(uint16_t)));
            h->allocs.push_back(dp);
            HIP_TRY(hipMemcpy(dp, t16.data(), t16.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
            E.d_emb16 = static_cast<uint16_t*>(dp);
        }
        int i = 0;
        for (const char* n : {"norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"})
            if ((rc = upload(h, g->weights.data(b + n), &E.d_ln[i++])) != HIFICAR_OK) return rc;
    }
    HIP_TRY(xfmr_for_every_d([](auto D) { return xfmr_attn_attr<D()>(); }));
    if (xfmr_arith(g->precision).a) HIP_TRY(xfmr_for_every_d([](auto D) { return xfmr_attn16_attr<D()>(); }));
    // the engine opens here, not in hificar_xfmr_create: a handle can be created and described without a device
    if ((rc = engine_open(h, true)) != HIFICAR_OK) return rc;
    h->precision = xfmr_x3(g) ? HIFICAR_PREC_BF16X3 : HIFICAR_PREC_F32;
    h->use_pair = false;
    h->ksplit = 0;  // one accumulation order for every launch shape: an utterance's result does not depend on what it is batched with
    HIP_TRY(hipDeviceSynchronize());
    g->weights.clear_staged();  // (g->weights.expected stays: the training entry points go by it)
    g->finalized = true;
    return HIFICAR_OK;
}

struct XfmrWorkspace {
    float* xin;     // [rows][cin_pad]
    float* r[5];    // [rows][F]; r[3] and r[4] in bf16x3 only (null otherwise)
    float* wide;    // [rows][3072]
    size_t bytes;
};

static XfmrWorkspace xfmr_plan_workspace(const hificar_xfmr* g, int B, int T, void* base) {
    const size_t rows = round_up_sz((size_t)std::max(B, 0) * (size_t)std::max(T, 0), 256);  // whole tiles of slack behind the last row
    XfmrWorkspace w;
    Carver cv(base, 256);
    w.xin = cv.floats(rows * g->cin_pad);
    // bf16x3: split rows take a fp32 row's bytes, and the layer input and norm1's output exist in both formats at once: two more row buffers
    const int nr = xfmr_x3(g) ? 5 : 3;
    for (int i = 0; i < 5; ++i) w.r[i] = i < nr ? cv.floats(rows * g->cfg.hidden_dim) : nullptr;
    w.wide = cv.floats(rows * kXfmrFF);
    w.bytes = cv.bytes();
    return w;
}

extern "C" size_t hificar_xfmr_workspace_bytes(const hificar_xfmr* g, int B, int T) {
    if (!g || B < 1 || T < 1) return 0;
    return xfmr_plan_workspace(g, B, T, nullptr).bytes;
}

// Test aid: the next forwards copy the named intermediate, as rows (B, T, hidden_dim), into dst (capacity in floats).  Names: "conv_blocks",
// "w_raw_in", "layers.<n>.norm1" (the attention sub-block's output), "layers.<n>" (the layer's output).  name = NULL: forget all; dst = NULL: forget one.
extern "C" int hificar_xfmr_debug_tap(hificar_xfmr* g, const char* name, float* dst, size_t capacity) {
    if (!g) return fail(HIFICAR_E_INVALID, "null handle");
    if (name && dst && xfmr_x3(g) && std::string(name) == "conv_blocks")
        return fail(HIFICAR_E_INVALID, "debug tap 'conv_blocks': a bf16x3 handle holds the conv blocks' output as split bf16 rows only, not as fp32 rows");
    g->taps.set(name, dst, capacity);
    return HIFICAR_OK;
}

static int xfmr_emit_tap(hificar_xfmr* g, const std::string& name, const float* rows, size_t floats, hipStream_t stream) {
    float* dst;
    const int rc = g->taps.find(name, floats, &dst);
    if (rc != HIFICAR_OK || !dst) return rc;
    HIP_TRY(hipMemcpyAsync(dst, rows, floats * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return HIFICAR_OK;
}

// The low-rate front end in place of xfmr_rows_kernel (hificar_xfmr_forward_lowrate): x is (B, in_channels, Tl) with `lengths` low-rate frame
// counts; everything behind the input rows goes by the frame counts at the model's rate.
struct XfmrFront {
    int Tl, factor;
    const int32_t* lengths;  // low-rate, device (or null)
    const double* stats;     // [B][mean, 1 / std], or null
};

// Every launch of the eval forward, after the arguments were checked and the stream entered.  lengths: at the model's rate.
static int xfmr_forward_run(hificar_xfmr* g, const float* x, const int32_t* lengths, float* out, int B, int T, const XfmrWorkspace& ws, hipStream_t stream,
                            const XfmrFront* fe) {
    hificar_engine* h = &g->eng;
    int rc;
    const int F = g->cfg.hidden_dim, C = g->cfg.in_channels, O = g->cfg.out_channels, d = F / kXfmrHeads;
    const double M = (double)B * T;
    const size_t MF = (size_t)B * T * F;
    Ragged rg;
    rg.seq_len = lengths;
    rg.frames = T;
    const bool x3 = xfmr_x3(g), a16 = xfmr_arith(g->precision).a;
    if (x3 && g->taps.wanted("conv_blocks")) return fail(HIFICAR_E_INVALID, "debug tap 'conv_blocks': a bf16x3 handle holds these rows as split bf16 rows only");
    // one launch of one layer: xs -> y (fp32) and / or ys (the activated copy: ReLU, or with slope 1 the identity), + res.  xs and ys are fp32
    // rows in exact fp32 and split rows in bf16x3; res_relu (bf16x3): res holds the rows before their ReLU
    auto conv = [&](const ConvLayer& L, const float* xs, const float* res, float* y, float* ys, float slope = 0.f, bool res_relu = false) {
        ConvIO io{};
        io.xs = reinterpret_cast<const char*>(xs);
        io.res = res;
        io.y = y;
        io.ys = reinterpret_cast<char*>(ys);
        io.res_relu = res_relu;
        return launch_conv1(h, L, B, T, io, slope, rg, stream);
    };
    // dst: the fp32 rows; dst_s (bf16x3): the same rows as split rows, the next GEMM's input
    auto layer_norm = [&](const float* src, const float* gamma, const float* beta, float* dst, float* dst_s) {
        XfmrLnParams p;
        p.x = src;
        p.gamma = gamma;
        p.beta = beta;
        p.lengths = lengths;
        p.y = dst;
        p.ys = reinterpret_cast<char*>(dst_s);
        p.B = B;
        p.T = T;
        p.F = F;
        ProfScope prof(h, stream, dst_s ? "xfmr_ln_kernel<split>" : "xfmr_ln_kernel", 8.0 * M * F, (dst_s ? 12.0 : 8.0) * M * F);
        const dim3 grid((unsigned)(((long long)B * T + 3) / 4));
        if (dst_s) hipLaunchKernelGGL(xfmr_ln_kernel<true>, grid, dim3(256), 0, stream, p);
        else hipLaunchKernelGGL(xfmr_ln_kernel<false>, grid, dim3(256), 0, stream, p);
        return hipGetLastError();
    };
    const bool has_rp = g->rp.cout != 0;
    {
        const dim3 grid((unsigned)((T + 31) / 32), (unsigned)(g->cin_pad / 32), (unsigned)B);
        if (fe) {  // (the same rows, formed from the low-rate input: hificar_frontend_kernels.hip.h)
            const double Ml = (double)B * fe->Tl;
            ProfScope prof(h, stream, x3 ? "frontend_rows_kernel<split>" : "frontend_rows_kernel", 0.0,
                           4.0 * (Ml * C + M * g->cin_pad * (x3 && !has_rp ? 2 : 1)));
            if (x3)
                hipLaunchKernelGGL(frontend_rows_kernel<true>, grid, dim3(256), 0, stream, x, has_rp ? nullptr : ws.r[1], reinterpret_cast<char*>(ws.xin),
                                   fe->lengths, fe->stats, C, g->cin_pad, fe->Tl, fe->factor);
            else
                hipLaunchKernelGGL(frontend_rows_kernel<false>, grid, dim3(256), 0, stream, x, ws.xin, static_cast<char*>(nullptr), fe->lengths, fe->stats, C,
                                   g->cin_pad, fe->Tl, fe->factor);
        } else if (x3) {  // (no residual_path: block 0's conv2 takes the input as its fp32 residual, kept in r[1])
            ProfScope prof(h, stream, "xfmr_rows_split_kernel", 0.0, 4.0 * M * (C + g->cin_pad * (has_rp ? 1 : 2)));
            hipLaunchKernelGGL(xfmr_rows_split_kernel, grid, dim3(256), 0, stream, x, reinterpret_cast<char*>(ws.xin), has_rp ? nullptr : ws.r[1], lengths, C,
                               g->cin_pad, T);
        } else {
            ProfScope prof(h, stream, "xfmr_rows_kernel", 0.0, 4.0 * M * (C + g->cin_pad));
            hipLaunchKernelGGL(xfmr_rows_kernel, grid, dim3(256), 0, stream, x, ws.xin, lengths, C, g->cin_pad, T, nullptr);
        }
        HIP_TRY(hipGetLastError());
    }
    // conv_blocks.  `in`: the block's input as conv1's operand; `res`: the same values as conv2's fp32 residual (block 0: residual_path's output).
    // Exact fp32: one buffer is both — a conv2 writes only the ReLU'd sum (ys), into r[2] (blocks 0 and 2) or r[1] (block 1).
    // bf16x3: the operand is split rows, so a conv2 writes the ReLU'd sum as split rows (ys: r[3], block 1: r[4]) and the sum BEFORE the ReLU as
    // fp32 rows (y: r[1] / r[2]), which the next conv2 ReLUs as it reads its residual.  r[0] holds conv1's ReLU'd output.
    const float* in = ws.xin;
    const float* res = x3 ? ws.r[1] : ws.xin;
    for (int i = 0; i < 3; ++i) {
        if ((rc = conv(g->c1[i], in, nullptr, nullptr, ws.r[0])) != HIFICAR_OK) return rc;
        if (i == 0 && has_rp) {
            if ((rc = conv(g->rp, in, nullptr, ws.r[1], nullptr)) != HIFICAR_OK) return rc;
            res = ws.r[1];
        }
        float* const ys = x3 ? (i == 1 ? ws.r[4] : ws.r[3]) : (i == 1 ? ws.r[1] : ws.r[2]);
        float* const y = x3 && i < 2 ? (res == ws.r[1] ? ws.r[2] : ws.r[1]) : nullptr;
        if ((rc = conv(g->c2[i], ws.r[0], res, y, ys, 0.f, x3 && i > 0)) != HIFICAR_OK) return rc;
        in = ys;
        res = x3 ? y : ys;
    }
    if (!x3 && (rc = xfmr_emit_tap(g, "conv_blocks", in, MF, stream)) != HIFICAR_OK) return rc;
    float* const X = ws.r[0];                     // the layer input, fp32 rows; r[1] and r[2] are free from here on
    float* const Xs = x3 ? ws.r[4] : nullptr;     // bf16x3: ... and its split copy (r[3], w_raw_in's operand, is free after this launch)
    // (bf16x3: slope 1 makes the activated copy the identity — w_raw_in's output is q | k | v's operand un-activated)
    if ((rc = conv(g->w_in, in, nullptr, X, Xs, x3 ? 1.f : 0.f)) != HIFICAR_OK) return rc;
    if ((rc = xfmr_emit_tap(g, "w_raw_in", X, MF, stream)) != HIFICAR_OK) return rc;
    float* const Ns = x3 ? ws.r[3] : nullptr;  // norm1's output as split rows
    for (int l = 0; l < g->cfg.elayers; ++l) {
        const XfmrEncLayer& E = g->enc[(size_t)l];
        const std::string name = "layers." + std::to_string(l);
        // (bf16x3a: q | k | v as split rows only — slope 1 is the identity copy — for the attention's MFMAs)
        if ((rc = a16 ? conv(E.qkv, Xs, nullptr, nullptr, ws.wide, 1.f) : conv(E.qkv, x3 ? Xs : X, nullptr, ws.wide, nullptr)) != HIFICAR_OK) return rc;
        if (a16) {
            XfmrAttn16Params p;
            p.qkv = reinterpret_cast<const char*>(ws.wide);
            p.tab = xfmr_tab16(E.d_emb16, d);
            p.lengths = lengths;
            p.out = reinterpret_cast<char*>(ws.r[1]);
            p.T = T;
            p.F = F;
            p.scale = (float)(1.0 / std::sqrt((double)d));
            ProfScope prof(h, stream, "xfmr_attn16_kernel", 2.0 * M * F * 3 * kXfmrTab, 4.0 * M * 4 * F);
            const dim3 grid((unsigned)((T + kXfmrTQ - 1) / kXfmrTQ), kXfmrHeads, (unsigned)B);
            const hipError_t e = xfmr_by_d(d, [&](auto D) { return xfmr_launch(xfmr_attn16_kernel<D()>, grid, XfmrAttn16Lds<D()>::bytes, stream, p); });
            if (e != hipSuccess) return fail(HIFICAR_E_HIP, "xfmr_attn16_kernel launch failed: %s", hipGetErrorString(e));
        } else {
            XfmrAttnParams p;
            p.qkv = ws.wide;
            p.emb = E.d_emb;
            p.lengths = lengths;
            p.out = ws.r[1];
            p.T = T;
            p.F = F;
            p.scale = (float)(1.0 / std::sqrt((double)d));
            // per query at most 199 keys: Q K^T, the positional product and P V
            ProfScope prof(h, stream, x3 ? "xfmr_attn_kernel<split>" : "xfmr_attn_kernel", 2.0 * M * F * 3 * kXfmrTab, 4.0 * M * 4 * F);
            const dim3 grid((unsigned)((T + kXfmrTQ - 1) / kXfmrTQ), kXfmrHeads, (unsigned)B);
            // (bf16x3: the instantiation that stores split rows)
            const hipError_t e = xfmr_by_d(d, [&](auto D) {
                return xfmr_launch(x3 ? xfmr_attn_kernel<D(), false, true> : xfmr_attn_kernel<D()>, grid, XfmrAttnLds<D()>::bytes, stream, p);
            });
            if (e != hipSuccess) return fail(HIFICAR_E_HIP, "xfmr_attn_kernel launch failed: %s", hipGetErrorString(e));
        }
        if ((rc = conv(E.wo, ws.r[1], X, ws.r[2], nullptr)) != HIFICAR_OK) return rc;
        HIP_TRY(layer_norm(ws.r[2], E.d_ln[0], E.d_ln[1], ws.r[1], Ns));
        if ((rc = xfmr_emit_tap(g, name + ".norm1", ws.r[1], MF, stream)) != HIFICAR_OK) return rc;
        if ((rc = conv(E.l1, x3 ? Ns : ws.r[1], nullptr, nullptr, ws.wide)) != HIFICAR_OK) return rc;
        if ((rc = conv(E.l2, ws.wide, ws.r[1], ws.r[2], nullptr)) != HIFICAR_OK) return rc;
        HIP_TRY(layer_norm(ws.r[2], E.d_ln[2], E.d_ln[3], X, Xs));
        if ((rc = xfmr_emit_tap(g, name, X, MF, stream)) != HIFICAR_OK) return rc;
    }
    if ((rc = conv(g->w_out, x3 ? Xs : X, nullptr, ws.wide, nullptr)) != HIFICAR_OK) return rc;
    {
        const int Op = g->w_out.cout_pad;
        ProfScope prof(h, stream, "xfmr_out_kernel", 0.0, 4.0 * M * (O + Op));
        hipLaunchKernelGGL(xfmr_out_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)(Op / 32), (unsigned)B), dim3(256), 0, stream, ws.wide, out, lengths, O,
                           Op, T, nullptr);
        HIP_TRY(hipGetLastError());
    }
    return HIFICAR_OK;
}

extern "C" int hificar_xfmr_forward(hificar_xfmr* g, const float* x, const int32_t* lengths, const int32_t* lengths_host, float* out, int B, int T,
                                    void* workspace, size_t workspace_bytes, void* stream_) {
    if (!g || !x || !out) return fail(HIFICAR_E_INVALID, "hificar_xfmr_forward: null argument");
    if (!g->finalized) return fail(HIFICAR_E_STATE, "hificar_xfmr_forward before hificar_xfmr_finalize");
    if (B < 1 || T < 1 || B > 65535 || (long long)B * T > (1LL << 30) / 8 || (long long)B * T * kXfmrFF >= (1LL << 31))
        return fail(HIFICAR_E_INVALID, "hificar_xfmr_forward: B=%d, T=%d out of range (B T 3072 < 2^31)", B, T);
    if (lengths_host && !lengths) return fail(HIFICAR_E_INVALID, "hificar_xfmr_forward: lengths_host without the device copy");
    if (lengths_host)
        for (int b = 0; b < B; ++b)
            if (lengths_host[b] < 0 || lengths_host[b] > T)
                return fail(HIFICAR_E_INVALID, "hificar_xfmr_forward: lengths[%d]=%d outside 0 .. T=%d", b, lengths_host[b], T);
    const XfmrWorkspace ws = xfmr_plan_workspace(g, B, T, workspace);
    int rc;
    if ((rc = check_workspace(nullptr, workspace, workspace_bytes, ws.bytes)) != HIFICAR_OK) return rc;
    hificar_engine* h = &g->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    return xfmr_forward_run(g, x, lengths, out, B, T, ws, stream, nullptr);
}

// ---- The low-rate front end (egs/ema/voc1/local/predict_ema.py:83-101): the input rows are formed from features at 1 / factor of the model's
// rate, z-scored per utterance if asked; every launch behind them is hificar_xfmr_forward's.
struct XfmrLowWorkspace {
    double* stats;  // [B][mean, 1 / std]
    int* lens;      // [B]: factor * lengths[b]
    size_t bytes;   // behind xfmr_plan_workspace(B, factor Tl)
};

static XfmrLowWorkspace xfmr_plan_workspace_lowrate(const hificar_xfmr* g, int B, int Tl, int factor, void* base) {
    XfmrLowWorkspace w;
    Carver cv(base, 256);
    cv.take<char>(xfmr_plan_workspace(g, B, Tl * factor, nullptr).bytes);  // (the forward's own buffers, carved by xfmr_plan_workspace)
    w.stats = cv.take<double>((size_t)std::max(B, 0) * 2 * sizeof(double));
    w.lens = cv.take<int>((size_t)std::max(B, 0) * sizeof(int));
    w.bytes = cv.bytes();
    return w;
}

static bool xfmr_lowrate_shape_ok(int B, int Tl, int factor) {
    const long long M = (long long)B * Tl * factor;
    return B >= 1 && Tl >= 1 && B <= 65535 && factor >= 1 && factor <= HIFICAR_LOWRATE_MAX_FACTOR && M <= (1LL << 30) / 8 && M * kXfmrFF < (1LL << 31);
}

extern "C" size_t hificar_xfmr_workspace_bytes_lowrate(const hificar_xfmr* g, int B, int Tl, int factor) {
    if (!g || !xfmr_lowrate_shape_ok(B, Tl, factor)) return 0;
    return xfmr_plan_workspace_lowrate(g, B, Tl, factor, nullptr).bytes;
}

extern "C" int hificar_xfmr_forward_lowrate(hificar_xfmr* g, const float* x, const int32_t* lengths, const int32_t* lengths_host, float* out, int B, int Tl,
                                            int factor, int zscore, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!g || !x || !out) return fail(HIFICAR_E_INVALID, "hificar_xfmr_forward_lowrate: null argument");
    if (factor < 1 || factor > HIFICAR_LOWRATE_MAX_FACTOR)
        return fail(HIFICAR_E_INVALID, "hificar_xfmr_forward_lowrate: factor=%d out of range (1 .. %d)", factor, HIFICAR_LOWRATE_MAX_FACTOR);
    if (!xfmr_lowrate_shape_ok(B, Tl, factor))
        return fail(HIFICAR_E_INVALID, "hificar_xfmr_forward_lowrate: B=%d, Tl=%d, factor=%d out of range (B factor Tl 3072 < 2^31)", B, Tl, factor);
    if (lengths_host && !lengths) return fail(HIFICAR_E_INVALID, "hificar_xfmr_forward_lowrate: lengths_host without the device copy");
    if (lengths_host)
        for (int b = 0; b < B; ++b)
            if (lengths_host[b] < 0 || lengths_host[b] > Tl)
                return fail(HIFICAR_E_INVALID, "hificar_xfmr_forward_lowrate: lengths[%d]=%d outside 0 .. Tl=%d", b, lengths_host[b], Tl);
    const XfmrLowWorkspace lw = xfmr_plan_workspace_lowrate(g, B, Tl, factor, workspace);
    int rc;
    if ((rc = check_workspace(nullptr, workspace, workspace_bytes, lw.bytes)) != HIFICAR_OK) return rc;
    // (every argument above is checked without the device: a handle that was never finalized is told so last)
    if (!g->finalized) return fail(HIFICAR_E_STATE, "hificar_xfmr_forward_lowrate before hificar_xfmr_finalize");
    if (factor == 1 && !zscore) return hificar_xfmr_forward(g, x, lengths, lengths_host, out, B, Tl, workspace, workspace_bytes, stream_);
    const int T = Tl * factor;
    const XfmrWorkspace ws = xfmr_plan_workspace(g, B, T, workspace);
    hificar_engine* h = &g->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    XfmrFront fe;
    fe.Tl = Tl;
    fe.factor = factor;
    fe.lengths = lengths;
    fe.stats = nullptr;
    const int32_t* lens_h = nullptr;
    if (lengths) {
        hipLaunchKernelGGL(frontend_lengths_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, lengths, lw.lens, B, Tl, factor);
        HIP_TRY(hipGetLastError());
        lens_h = lw.lens;
    }
    if (zscore) {
        ProfScope prof(h, stream, "frontend_stats_kernel", 0.0, 8.0 * B * Tl * g->cfg.in_channels);
        hipLaunchKernelGGL(frontend_stats_kernel, dim3((unsigned)B), dim3(256), 0, stream, x, lengths, lw.stats, g->cfg.in_channels, Tl);
        HIP_TRY(hipGetLastError());
        fe.stats = lw.stats;
    }
    return xfmr_forward_run(g, x, lens_h, out, B, T, ws, stream, &fe);
}
