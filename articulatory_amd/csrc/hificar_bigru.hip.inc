// The BiGRU articulatory-inversion model (articulatory/models/pytorch_models.py:22-123): features (B, in_channels, T) -> EMA (B, out_channels, T).
//   rows      (B, C, T) -> channels-last rows                                   bigru_rows_kernel
//   gru1/2    pre-gates  X W_ih^T + b_ih, both directions in one GEMM (N = 6H)   conv engine, one-tap launch (as the discriminators' GEMMs)
//             the recurrent sweep, one workgroup per (direction, sequence tile)  bigru_rec_kernel
//   fc1 + bn  Linear(2H, 128) with the eval-mode BatchNorm1d folded in           conv engine
//   fc2       Linear(128, out) (+ tanh), written as (B, out, T)                  bigru_head_kernel
// Workspace: one pre-gate buffer [B T][6H] shared by the two layers (and by fc1's output), one row buffer [B T][max(Cin, 2H)] shared by
// the input rows and the two layers' hidden states.  Exact fp32.

struct BigruTrain;  // training state (hificar_bigru_train.hip.inc): made by the first training entry point

struct hificar_bigru {
    hificar_bigru_config cfg;
    hificar_engine eng;
    WeightIntake weights;
    ConvLayer proj[2], fc1;
    float4* d_whh[2] = {nullptr, nullptr};  // [dir][3 * H/8][2H] float4 per layer (BigruSplit)
    float* d_bhh[2] = {nullptr, nullptr};   // [dir][3H] per layer
    float* d_w2 = nullptr;
    float* d_b2 = nullptr;
    int cin_pad = 0;
    bool finalized = false;
    BigruTrain* train = nullptr;
    int train_failed = HIFICAR_OK;  // the error of a failed set-up of the training state: it is not tried again on this handle
};

static void bigru_train_free(hificar_bigru* g);

static std::string bigru_fc2_name(const hificar_bigru* g) { return g->cfg.use_tanh ? "fc2.0" : "fc2"; }

extern "C" int hificar_bigru_create(const hificar_bigru_config* cfg, hificar_bigru** out) {
    if (!cfg || !out) return fail(HIFICAR_E_INVALID, "hificar_bigru_create: null argument");
    const hificar_bigru_config& c = *cfg;
    if (c.in_channels < 1 || c.in_channels > HIFICAR_BIGRU_MAX_IN)
        return fail(HIFICAR_E_INVALID, "BiGRU: in_channels=%d out of range (1 .. %d)", c.in_channels, HIFICAR_BIGRU_MAX_IN);
    if (c.hidden_size < 64 || c.hidden_size > HIFICAR_BIGRU_MAX_HIDDEN || c.hidden_size % 64 != 0)
        return fail(HIFICAR_E_INVALID, "BiGRU: hidden_size=%d unsupported (multiples of 64 up to %d: one workgroup holds a direction's W_hh)",
                    c.hidden_size, HIFICAR_BIGRU_MAX_HIDDEN);
    if (c.out_channels < 1 || c.out_channels > HIFICAR_BIGRU_MAX_OUT)
        return fail(HIFICAR_E_INVALID, "BiGRU: out_channels=%d out of range (1 .. %d)", c.out_channels, HIFICAR_BIGRU_MAX_OUT);
    static_assert(HIFICAR_BIGRU_MAX_OUT == kBigruMaxOut, "head kernel's LDS table");
    hificar_bigru* g = new hificar_bigru();
    g->cfg = c;
    const int64_t H = c.hidden_size, C = c.in_channels, O = c.out_channels;
    g->cin_pad = round_up(c.in_channels, 32);
    for (int l = 1; l <= 2; ++l)
        for (const char* sfx : {"", "_reverse"}) {
            const std::string b = "gru" + std::to_string(l) + ".";
            g->weights.expected[b + "weight_ih_l0" + sfx] = {3 * H, l == 1 ? C : 2 * H};
            g->weights.expected[b + "weight_hh_l0" + sfx] = {3 * H, H};
            g->weights.expected[b + "bias_ih_l0" + sfx] = {3 * H};
            g->weights.expected[b + "bias_hh_l0" + sfx] = {3 * H};
        }
    g->weights.expected["fc1.0.weight"] = {kBigruFc1, 2 * H};
    g->weights.expected["fc1.0.bias"] = {kBigruFc1};
    for (const char* n : {"bn.weight", "bn.bias", "bn.running_mean", "bn.running_var"}) g->weights.expected[n] = {kBigruFc1};
    g->weights.expected[bigru_fc2_name(g) + ".weight"] = {O, kBigruFc1};
    g->weights.expected[bigru_fc2_name(g) + ".bias"] = {O};
    int rc = HIFICAR_OK;
    for (int l = 0; l < 2 && rc == HIFICAR_OK; ++l) {
        ConvLayer& P = g->proj[l];
        P.name = "gru" + std::to_string(l + 1) + "#proj";
        P.cin = l == 0 ? c.in_channels : 2 * c.hidden_size;
        P.cin_pad = l == 0 ? g->cin_pad : 2 * c.hidden_size;
        P.cout = 6 * c.hidden_size;
        P.K = 1;
        rc = plan_layer(P);
    }
    if (rc == HIFICAR_OK) {
        ConvLayer& F = g->fc1;
        F.name = "fc1#bn";
        F.cin = F.cin_pad = 2 * c.hidden_size;
        F.cout = kBigruFc1;
        F.K = 1;
        rc = plan_layer(F);
    }
    if (rc != HIFICAR_OK) {
        delete g;
        return rc;
    }
    *out = g;
    return HIFICAR_OK;
}

extern "C" void hificar_bigru_destroy(hificar_bigru* g) {
    if (!g) return;
    bigru_train_free(g);
    engine_close(&g->eng);
    delete g;
}

extern "C" hificar_engine* hificar_bigru_engine(hificar_bigru* g) { return g ? &g->eng : nullptr; }

extern "C" int hificar_bigru_set_weight(hificar_bigru* g, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!g || !name || !data || !shape) return fail(HIFICAR_E_INVALID, "hificar_bigru_set_weight: null argument");
    if (g->finalized) return fail(HIFICAR_E_STATE, "hificar_bigru_set_weight(%s) after hificar_bigru_finalize", name);
    return g->weights.set(name, data, shape, ndim);
}

// W_hh of both directions in the recurrent kernel's order: [dir][gate * H/8 + column][thread 2 i + q] float4 = W_hh[gate H + i][q H/2 + 4 column ..]
static std::vector<float> bigru_pack_whh(const HostTensor& fwd, const HostTensor& rev, int H) {
    const int NT = 2 * H, KH = H / 2, CH = KH / 4;
    std::vector<float> w((size_t)2 * 3 * CH * NT * 4);
    for (int dir = 0; dir < 2; ++dir) {
        const std::vector<float>& src = (dir ? rev : fwd).data;
        for (int gt = 0; gt < 3; ++gt)
            for (int c = 0; c < CH; ++c)
                for (int tid = 0; tid < NT; ++tid) {
                    const int i = tid >> 1, q = tid & 1;
                    float* dst = &w[((((size_t)dir * 3 + gt) * CH + c) * NT + tid) * 4];
                    for (int e = 0; e < 4; ++e) dst[e] = src[(size_t)(gt * H + i) * H + q * KH + 4 * c + e];
                }
    }
    return w;
}

template <int H, int NS>
static hipError_t bigru_rec_attr() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&bigru_rec_kernel<H, NS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)BigruSplit<H, NS>::lds_bytes);
}

template <int H, int NS>
static hipError_t bigru_rec_launch_one(const BigruRecParams& p, hipStream_t stream) {
    const dim3 grid((unsigned)((p.B + NS - 1) / NS), 2, 1);
    constexpr size_t lds = BigruSplit<H, NS>::lds_bytes;
    hipLaunchKernelGGL((bigru_rec_kernel<H, NS>), grid, dim3(2 * H), lds, stream, p);
    return hipGetLastError();
}

template <int NS>
static hipError_t bigru_rec_launch_h(int H, const BigruRecParams& p, hipStream_t stream) {
    switch (H) {
        case 64: return bigru_rec_launch_one<64, NS>(p, stream);
        case 128: return bigru_rec_launch_one<128, NS>(p, stream);
        case 192: return bigru_rec_launch_one<192, NS>(p, stream);
        case 256: return bigru_rec_launch_one<256, NS>(p, stream);
    }
    return hipErrorInvalidValue;
}

// Sequences per workgroup: one while 2 B workgroups fit the chip (a sequence alone is the fastest sweep: most of W_hh in registers), two beyond.
static int bigru_tile_height(const hificar_bigru* g, int B) {
    if (const char* e = getenv("HIFICAR_BIGRU_NS")) {  // A/B runs of the choice (tools/bigru_bench.py)
        const int v = atoi(e);
        if (v == 1 || v == 2) return v;
    }
    return 2 * B <= g->eng.num_cus ? 1 : 2;
}

extern "C" int hificar_bigru_finalize(hificar_bigru* g) {
    if (!g) return fail(HIFICAR_E_INVALID, "hificar_bigru_finalize: null handle");
    if (g->finalized) return HIFICAR_OK;
    if (const int missing = g->weights.check_complete()) return missing;
    hificar_engine* h = &g->eng;
    const int H = g->cfg.hidden_size, O = g->cfg.out_channels;
    int rc;
    for (int l = 0; l < 2; ++l) {
        const std::string b = "gru" + std::to_string(l + 1) + ".";
        ConvLayer& P = g->proj[l];
        HostTensor W, Bv;  // (6H, Cin, 1): forward rows, then reverse rows
        W.shape = {6 * H, P.cin, 1};
        for (const char* sfx : {"", "_reverse"}) {
            const HostTensor& wi = g->weights.at(b + "weight_ih_l0" + sfx);
            const HostTensor& bi = g->weights.at(b + "bias_ih_l0" + sfx);
            W.data.insert(W.data.end(), wi.data.begin(), wi.data.end());
            Bv.data.insert(Bv.data.end(), bi.data.begin(), bi.data.end());
        }
        Bv.shape = {6 * H};
        if ((rc = pack_conv(h, P, W, &Bv)) != HIFICAR_OK) return rc;
        float* whh = nullptr;
        if ((rc = upload(h, bigru_pack_whh(g->weights.at(b + "weight_hh_l0"), g->weights.at(b + "weight_hh_l0_reverse"), H), &whh)) != HIFICAR_OK) return rc;
        g->d_whh[l] = reinterpret_cast<float4*>(whh);
        std::vector<float> bhh = g->weights.data(b + "bias_hh_l0");
        const std::vector<float>& br = g->weights.data(b + "bias_hh_l0_reverse");
        bhh.insert(bhh.end(), br.begin(), br.end());
        if ((rc = upload(h, bhh, &g->d_bhh[l])) != HIFICAR_OK) return rc;
    }
    {   // fc1 with the eval-mode batch norm folded in: y = (W x + b - mean) * gamma / sqrt(var + 1e-5) + beta  (pytorch_models.py:68-70)
        const HostTensor& W = g->weights.at("fc1.0.weight");
        const std::vector<float>&b1 = g->weights.data("fc1.0.bias"), &gm = g->weights.data("bn.weight"), &bt = g->weights.data("bn.bias"),
                         &mu = g->weights.data("bn.running_mean"), &var = g->weights.data("bn.running_var");
        HostTensor Wf, Bf;
        Wf.shape = {kBigruFc1, 2 * H, 1};
        Wf.data.resize(W.data.size());
        Bf.shape = {kBigruFc1};
        Bf.data.resize(kBigruFc1);
        for (int o = 0; o < kBigruFc1; ++o) {
            const double s = (double)gm[o] / std::sqrt((double)var[o] + 1e-5);
            for (int k = 0; k < 2 * H; ++k) Wf.data[(size_t)o * 2 * H + k] = (float)((double)W.data[(size_t)o * 2 * H + k] * s);
            Bf.data[o] = (float)(((double)b1[o] - (double)mu[o]) * s + (double)bt[o]);
        }
        if ((rc = pack_conv(h, g->fc1, Wf, &Bf)) != HIFICAR_OK) return rc;
    }
    if ((rc = upload(h, g->weights.data(bigru_fc2_name(g) + ".weight"), &g->d_w2)) != HIFICAR_OK) return rc;
    if ((rc = upload(h, g->weights.data(bigru_fc2_name(g) + ".bias"), &g->d_b2)) != HIFICAR_OK) return rc;
    (void)O;
    HIP_TRY((bigru_rec_attr<64, 1>()));
    HIP_TRY((bigru_rec_attr<64, 2>()));
    HIP_TRY((bigru_rec_attr<128, 1>()));
    HIP_TRY((bigru_rec_attr<128, 2>()));
    HIP_TRY((bigru_rec_attr<192, 1>()));
    HIP_TRY((bigru_rec_attr<192, 2>()));
    HIP_TRY((bigru_rec_attr<256, 1>()));
    HIP_TRY((bigru_rec_attr<256, 2>()));
    // the engine opens here, not in hificar_bigru_create: a handle can be created and described without a device
    if ((rc = engine_open(h, true)) != HIFICAR_OK) return rc;
    h->precision = HIFICAR_PREC_F32;
    h->use_pair = false;
    h->ksplit = 0;  // one accumulation order for every launch shape: an utterance's result does not depend on what it is batched with, bit
                    // for bit (the GEMMs are a few percent of a forward next to the sweeps, so the split-K form has nothing to win here)
    HIP_TRY(hipDeviceSynchronize());
    g->weights.clear_staged();
    g->finalized = true;
    return HIFICAR_OK;
}

struct BigruWorkspace {
    float* gates;  // [rows][6H]; fc1's output [rows][128] after the second sweep
    float* rows;   // [rows][max(cin_pad, 2H)]: input rows, then the layers' hidden states
    size_t bytes;
};

static BigruWorkspace bigru_plan_workspace(const hificar_bigru* g, int B, int T, void* base) {
    const size_t rows = round_up_sz((size_t)std::max(B, 0) * (size_t)std::max(T, 0), 256);  // whole tiles of slack behind the last row
    BigruWorkspace w;
    Carver cv(base, 256);
    w.gates = cv.floats(rows * 6 * g->cfg.hidden_size);
    w.rows = cv.floats(rows * std::max(g->cin_pad, 2 * g->cfg.hidden_size));
    w.bytes = cv.bytes();
    return w;
}

extern "C" size_t hificar_bigru_workspace_bytes(const hificar_bigru* g, int B, int T) {
    if (!g || B < 1 || T < 1) return 0;
    return bigru_plan_workspace(g, B, T, nullptr).bytes;
}

extern "C" int hificar_bigru_forward(hificar_bigru* g, const float* x, const int32_t* lengths, const int32_t* lengths_host, float* out, int B, int T,
                                     void* workspace, size_t workspace_bytes, void* stream_) {
    if (!g || !x || !out) return fail(HIFICAR_E_INVALID, "hificar_bigru_forward: null argument");
    if (!g->finalized) return fail(HIFICAR_E_STATE, "hificar_bigru_forward before hificar_bigru_finalize");
    if (B < 1 || T < 1 || B > 65535 || (long long)B * T > (1LL << 30) / 8)
        return fail(HIFICAR_E_INVALID, "hificar_bigru_forward: B=%d, T=%d out of range", B, T);
    if (lengths_host && !lengths) return fail(HIFICAR_E_INVALID, "hificar_bigru_forward: lengths_host without the device copy");
    if (lengths_host)
        for (int b = 0; b < B; ++b)
            if (lengths_host[b] < 0 || lengths_host[b] > T)
                return fail(HIFICAR_E_INVALID, "hificar_bigru_forward: lengths[%d]=%d outside 0 .. T=%d", b, lengths_host[b], T);
    const BigruWorkspace ws = bigru_plan_workspace(g, B, T, workspace);
    int rc;
    if ((rc = check_workspace(nullptr, workspace, workspace_bytes, ws.bytes)) != HIFICAR_OK) return rc;
    hificar_engine* h = &g->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    const int H = g->cfg.hidden_size, C = g->cfg.in_channels, O = g->cfg.out_channels, M = B * T;
    const Ragged rg;
    {
        ProfScope prof(h, stream, "bigru_rows_kernel", 0.0, 4.0 * M * (C + g->cin_pad));
        hipLaunchKernelGGL(bigru_rows_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)(g->cin_pad / 32), (unsigned)B), dim3(256), 0, stream, x, ws.rows, C,
                           g->cin_pad, T);
        HIP_TRY(hipGetLastError());
    }
    const int NS = bigru_tile_height(g, B);
    for (int l = 0; l < 2; ++l) {
        ConvIO io{};
        io.xs = reinterpret_cast<const char*>(ws.rows);
        io.y = ws.gates;
        if ((rc = launch_conv1(h, g->proj[l], 1, M, io, 0.f, rg, stream)) != HIFICAR_OK) return rc;
        BigruRecParams p;
        p.g = ws.gates;
        p.w = g->d_whh[l];
        p.bhh = g->d_bhh[l];
        p.lengths = lengths;
        p.y = ws.rows;  // (the projection that read the rows is complete: same stream)
        p.B = B;
        p.T = T;
        ProfScope prof(h, stream, "bigru_rec_kernel", 2.0 * M * 2 * 3 * H * H, 4.0 * M * 8 * H);
        const hipError_t e = NS == 1 ? bigru_rec_launch_h<1>(H, p, stream) : bigru_rec_launch_h<2>(H, p, stream);
        if (e != hipSuccess) return fail(HIFICAR_E_HIP, "bigru_rec_kernel launch failed: %s", hipGetErrorString(e));
    }
    {
        ConvIO io{};
        io.xs = reinterpret_cast<const char*>(ws.rows);
        io.y = ws.gates;
        if ((rc = launch_conv1(h, g->fc1, 1, M, io, 0.f, rg, stream)) != HIFICAR_OK) return rc;
    }
    {
        BigruHeadParams p;
        p.f = ws.gates;
        p.w2 = g->d_w2;
        p.b2 = g->d_b2;
        p.lengths = lengths;
        p.out = out;
        p.B = B;
        p.T = T;
        p.O = O;
        p.use_tanh = g->cfg.use_tanh;
        ProfScope prof(h, stream, "bigru_head_kernel", 2.0 * M * kBigruFc1 * O, 4.0 * M * (kBigruFc1 + O));
        hipLaunchKernelGGL(bigru_head_kernel, dim3((unsigned)((T + 63) / 64), (unsigned)B), dim3(256), 0, stream, p);
        HIP_TRY(hipGetLastError());
    }
    return HIFICAR_OK;
}

// ---- The low-rate front end (egs/ema/voc1/local/predict_ema.py:83-101): features at 1 / factor of the model's rate, and / or to be z-scored
// per utterance.  Linear interpolation is an affine combination whose weights sum to one, so interp(X) W_ih^T + b_ih = interp(X W_ih^T + b_ih):
// layer 1's projection runs over the B Tl low-rate rows and its 6H-wide pre-gates are interpolated (hificar_frontend_kernels.hip.h).  From
// the first sweep on the launches are hificar_bigru_forward's.
struct BigruLowWorkspace {
    float* gates;   // [B T rows][6H], as BigruWorkspace
    float* gates_l; // [B Tl rows][6H]: layer 1's pre-gates at the low rate (factor 1: null, the GEMM writes `gates`)
    float* rows;    // the low-rate input rows [B Tl rows][cin_pad], then the layers' hidden states [B T rows][2H]
    double* stats;  // [B][mean, 1 / std]
    int* lens;      // [B]: factor * lengths[b], what the sweeps and the head go by
    size_t bytes;
};

static BigruLowWorkspace bigru_plan_workspace_lowrate(const hificar_bigru* g, int B, int Tl, int factor, void* base) {
    const size_t rows_l = round_up_sz((size_t)std::max(B, 0) * (size_t)std::max(Tl, 0), 256);
    const size_t rows_h = round_up_sz((size_t)std::max(B, 0) * (size_t)std::max(Tl, 0) * (size_t)std::max(factor, 1), 256);
    const size_t H = (size_t)g->cfg.hidden_size;
    BigruLowWorkspace w;
    Carver cv(base, 256);
    w.gates = cv.floats(rows_h * 6 * H);
    w.gates_l = factor > 1 ? cv.floats(rows_l * 6 * H) : nullptr;
    w.rows = cv.floats(std::max(rows_l * (size_t)g->cin_pad, rows_h * 2 * H));
    w.stats = cv.take<double>((size_t)std::max(B, 0) * 2 * sizeof(double));
    w.lens = cv.take<int>((size_t)std::max(B, 0) * sizeof(int));
    w.bytes = cv.bytes();
    return w;
}

static bool lowrate_shape_ok(int B, int Tl, int factor) {
    return B >= 1 && Tl >= 1 && B <= 65535 && factor >= 1 && factor <= HIFICAR_LOWRATE_MAX_FACTOR && (long long)B * Tl * factor <= (1LL << 30) / 8;
}

extern "C" size_t hificar_bigru_workspace_bytes_lowrate(const hificar_bigru* g, int B, int Tl, int factor) {
    if (!g || !lowrate_shape_ok(B, Tl, factor)) return 0;
    // (factor 1 without zscore is hificar_bigru_forward on the same memory)
    return std::max(bigru_plan_workspace_lowrate(g, B, Tl, factor, nullptr).bytes, bigru_plan_workspace(g, B, Tl * factor, nullptr).bytes);
}

extern "C" int hificar_bigru_forward_lowrate(hificar_bigru* g, const float* x, const int32_t* lengths, const int32_t* lengths_host, float* out, int B, int Tl,
                                             int factor, int zscore, void* workspace, size_t workspace_bytes, void* stream_) {
    static_assert(HIFICAR_LOWRATE_MAX_FACTOR == kFrontMaxFactor, "the front end's tile");
    if (!g || !x || !out) return fail(HIFICAR_E_INVALID, "hificar_bigru_forward_lowrate: null argument");
    if (factor < 1 || factor > HIFICAR_LOWRATE_MAX_FACTOR)
        return fail(HIFICAR_E_INVALID, "hificar_bigru_forward_lowrate: factor=%d out of range (1 .. %d)", factor, HIFICAR_LOWRATE_MAX_FACTOR);
    if (!lowrate_shape_ok(B, Tl, factor)) return fail(HIFICAR_E_INVALID, "hificar_bigru_forward_lowrate: B=%d, Tl=%d, factor=%d out of range", B, Tl, factor);
    if (lengths_host && !lengths) return fail(HIFICAR_E_INVALID, "hificar_bigru_forward_lowrate: lengths_host without the device copy");
    if (lengths_host)
        for (int b = 0; b < B; ++b)
            if (lengths_host[b] < 0 || lengths_host[b] > Tl)
                return fail(HIFICAR_E_INVALID, "hificar_bigru_forward_lowrate: lengths[%d]=%d outside 0 .. Tl=%d", b, lengths_host[b], Tl);
    int rc;
    if ((rc = check_workspace(nullptr, workspace, workspace_bytes, hificar_bigru_workspace_bytes_lowrate(g, B, Tl, factor))) != HIFICAR_OK) return rc;
    // (every argument above is checked without the device: a handle that was never finalized is told so last)
    if (!g->finalized) return fail(HIFICAR_E_STATE, "hificar_bigru_forward_lowrate before hificar_bigru_finalize");
    if (factor == 1 && !zscore) return hificar_bigru_forward(g, x, lengths, lengths_host, out, B, Tl, workspace, workspace_bytes, stream_);
    const BigruLowWorkspace ws = bigru_plan_workspace_lowrate(g, B, Tl, factor, workspace);
    hificar_engine* h = &g->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    const int H = g->cfg.hidden_size, C = g->cfg.in_channels, O = g->cfg.out_channels, T = Tl * factor, Ml = B * Tl, M = B * T;
    const Ragged rg;
    const int* lens_h = nullptr;  // the frame counts at the model's rate
    if (lengths) {
        hipLaunchKernelGGL(frontend_lengths_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, lengths, ws.lens, B, Tl, factor);
        HIP_TRY(hipGetLastError());
        lens_h = ws.lens;
    }
    if (zscore) {
        ProfScope prof(h, stream, "frontend_stats_kernel", 0.0, 8.0 * Ml * C);
        hipLaunchKernelGGL(frontend_stats_kernel, dim3((unsigned)B), dim3(256), 0, stream, x, lengths, ws.stats, C, Tl);
        HIP_TRY(hipGetLastError());
    }
    {   // the input rows at the LOW rate: the interpolation commutes with the projection behind them
        ProfScope prof(h, stream, "frontend_rows_kernel", 0.0, 4.0 * Ml * (C + g->cin_pad));
        hipLaunchKernelGGL(frontend_rows_kernel<false>, dim3((unsigned)((Tl + 31) / 32), (unsigned)(g->cin_pad / 32), (unsigned)B), dim3(256), 0, stream, x, ws.rows,
                           static_cast<char*>(nullptr), lengths, zscore ? ws.stats : static_cast<const double*>(nullptr), C, g->cin_pad, Tl, 1);
        HIP_TRY(hipGetLastError());
    }
    const int NS = bigru_tile_height(g, B);
    for (int l = 0; l < 2; ++l) {
        ConvIO io{};
        io.xs = reinterpret_cast<const char*>(ws.rows);
        io.y = l == 0 && factor > 1 ? ws.gates_l : ws.gates;
        if ((rc = launch_conv1(h, g->proj[l], 1, l == 0 ? Ml : M, io, 0.f, rg, stream)) != HIFICAR_OK) return rc;
        if (l == 0 && factor > 1) {
            const int N4 = 6 * H / 4;
            ProfScope prof(h, stream, "bigru_interp_gates_kernel", 3.0 * M * 6 * H, 4.0 * M * 6 * H * 3);
            hipLaunchKernelGGL(bigru_interp_gates_kernel, dim3((unsigned)(((long long)T * N4 + 255) / 256), 1, (unsigned)B), dim3(256), 0, stream, ws.gates_l,
                               ws.gates, lengths, N4, Tl, factor);
            HIP_TRY(hipGetLastError());
        }
        BigruRecParams p;
        p.g = ws.gates;
        p.w = g->d_whh[l];
        p.bhh = g->d_bhh[l];
        p.lengths = lens_h;
        p.y = ws.rows;  // (the projection that read the rows is complete: same stream)
        p.B = B;
        p.T = T;
        ProfScope prof(h, stream, "bigru_rec_kernel", 2.0 * M * 2 * 3 * H * H, 4.0 * M * 8 * H);
        const hipError_t e = NS == 1 ? bigru_rec_launch_h<1>(H, p, stream) : bigru_rec_launch_h<2>(H, p, stream);
        if (e != hipSuccess) return fail(HIFICAR_E_HIP, "bigru_rec_kernel launch failed: %s", hipGetErrorString(e));
    }
    {
        ConvIO io{};
        io.xs = reinterpret_cast<const char*>(ws.rows);
        io.y = ws.gates;
        if ((rc = launch_conv1(h, g->fc1, 1, M, io, 0.f, rg, stream)) != HIFICAR_OK) return rc;
    }
    {
        BigruHeadParams p;
        p.f = ws.gates;
        p.w2 = g->d_w2;
        p.b2 = g->d_b2;
        p.lengths = lens_h;
        p.out = out;
        p.B = B;
        p.T = T;
        p.O = O;
        p.use_tanh = g->cfg.use_tanh;
        ProfScope prof(h, stream, "bigru_head_kernel", 2.0 * M * kBigruFc1 * O, 4.0 * M * (kBigruFc1 + O));
        hipLaunchKernelGGL(bigru_head_kernel, dim3((unsigned)((T + 63) / 64), (unsigned)B), dim3(256), 0, stream, p);
        HIP_TRY(hipGetLastError());
    }
    return HIFICAR_OK;
}
