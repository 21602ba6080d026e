// Training of the BiGRU inversion model (the reference's step: articulatory/bin/train.py:241-383 through pytorch_models.py:45-72 in
// train() mode): device-resident parameters, the training-mode forward with its tape, and the backward pass.
//   forward   rows -> [proj GEMM -> recurrent sweep (keeps r, z, n, W_hn h + b_hn) -> dropout] x 2 -> raw fc1 GEMM -> batch statistics
//             -> dropout + batch norm + fc2 (+ tanh) in the head kernel
//   backward  head (tanh', dW_fc2, db_fc2) -> batch norm + dropout -> fc1 (dW, db, dY2) -> [dropout mask -> backward sweep -> dW_ih, db_ih,
//             dW_hh, db_hh, dX] x 2 -> dx
// The GEMMs are the conv engine's one-tap launches (forward and data gradients) and the weight-gradient kernels of hificar_train.hip.inc.
// Ragged batches (hificar_bigru_forward_train_ragged): every sequence is swept over its own frame count, the batch statistics and every
// gradient take the valid frames only; the GEMMs still run over all B T rows, and zeros in the padded rows of their operands mask them.
// Low-rate inputs (hificar_bigru_forward_train_lowrate / hificar_bigru_backward_lowrate): the same step on x at 1 / factor of the model's rate;
// layer 1's projection and its gradients run over the B Tl low-rate rows, the interpolation and its adjoint stand between them and the sweeps.
// Kernels: hificar_bigru_train_kernels.hip.h, hificar_frontend_kernels.hip.h.

struct BigruTrain {
    FeatureParamTable tab;  // the master copy: the parameters, bn.running_mean / running_var, the folded fc1 (eval form)
    int64_t off_fold_w = 0, off_fold_b = 0;
    ConvLayer fc1_raw, hh;     // fc1 without the batch norm; the shape of one direction's W_hh for the weight-gradient kernels
    ConvLayer dg_proj[2], dg_fc1;
    float4* d_whht[2] = {nullptr, nullptr};  // W_hh transposed and packed for the backward sweep
    bool have_params = false;
};

static void bigru_train_free(hificar_bigru* g) {
    delete g->train;  // (device memory: the engine's allocation list)
    g->train = nullptr;
}

template <int H, int NS>
static hipError_t bigru_train_attr() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&bigru_rec_kernel<H, NS, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)BigruSplit<H, NS>::lds_bytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&bigru_rec_bwd_kernel<H, NS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(BigruSplit<H, NS>::lds_bytes + (size_t)4 * NS * H * 4));  // (da_r, da_z, dq) x 2 instead of h x 2
}

template <int H, int NS>
static hipError_t bigru_rec_train_launch_one(const BigruRecParams& p, hipStream_t stream) {
    constexpr size_t lds = BigruSplit<H, NS>::lds_bytes;
    hipLaunchKernelGGL((bigru_rec_kernel<H, NS, true>), dim3((unsigned)((p.B + NS - 1) / NS), 2, 1), dim3(2 * H), lds, stream, p);
    return hipGetLastError();
}

template <int H, int NS>
static hipError_t bigru_rec_bwd_launch_one(const BigruRecBwdParams& p, hipStream_t stream) {
    constexpr size_t lds = BigruSplit<H, NS>::lds_bytes + (size_t)4 * NS * H * 4;
    static_assert(lds <= 160 * 1024, "the backward sweep's LDS");
    hipLaunchKernelGGL((bigru_rec_bwd_kernel<H, NS>), dim3((unsigned)((p.B + NS - 1) / NS), 2, 1), dim3(2 * H), lds, stream, p);
    return hipGetLastError();
}

#define HIFICAR_BIGRU_BY_SHAPE(fn, H, NS, ...)                                   \
    ((NS) == 1 ? ((H) == 64 ? fn<64, 1>(__VA_ARGS__) : (H) == 128 ? fn<128, 1>(__VA_ARGS__) : (H) == 192 ? fn<192, 1>(__VA_ARGS__) : fn<256, 1>(__VA_ARGS__)) \
               : ((H) == 64 ? fn<64, 2>(__VA_ARGS__) : (H) == 128 ? fn<128, 2>(__VA_ARGS__) : (H) == 192 ? fn<192, 2>(__VA_ARGS__) : fn<256, 2>(__VA_ARGS__)))

static int bigru_train_build(hificar_bigru* g, BigruTrain* ts);

static int bigru_train_init(hificar_bigru* g) {
    if (g->train) return HIFICAR_OK;
    if (!g->finalized) return fail(HIFICAR_E_STATE, "BiGRU training entry points need hificar_bigru_finalize first");
    return feature_train_make(g, bigru_train_build, "BiGRU");
}

static int bigru_train_build(hificar_bigru* g, BigruTrain* ts) {
    hificar_engine* h = &g->eng;
    const int H = g->cfg.hidden_size;
    FeatureParamTable& tab = ts->tab;
    auto add = [&](const std::string& name, bool trainable) { tab.add(g->weights.expected, name, trainable); };
    // a layer's forward and reverse tensors of one kind lie back to back: (6H, Cin) / (6H) / 2 x (3H, H) blocks, as the GEMMs see them
    for (int l = 1; l <= 2; ++l) {
        const std::string b = "gru" + std::to_string(l) + ".";
        for (const char* kind : {"weight_ih_l0", "bias_ih_l0", "weight_hh_l0", "bias_hh_l0"})
            for (const char* sfx : {"", "_reverse"}) add(b + kind + sfx, true);
    }
    for (const char* n : {"fc1.0.weight", "fc1.0.bias", "bn.weight", "bn.bias"}) add(n, true);
    add(bigru_fc2_name(g) + ".weight", true);
    add(bigru_fc2_name(g) + ".bias", true);
    tab.grad_total = tab.master_total;
    add("bn.running_mean", false);
    add("bn.running_var", false);
    ts->off_fold_w = tab.reserve((int64_t)kBigruFc1 * 2 * H);
    ts->off_fold_b = tab.reserve(kBigruFc1);
    int rc;
    void* p = nullptr;
    if ((rc = feature_alloc(h, (size_t)tab.master_total * sizeof(float), &p)) != HIFICAR_OK) return rc;
    tab.d_master = static_cast<float*>(p);

    ConvLayer& F = ts->fc1_raw;
    F.name = "fc1#raw";
    F.cin = F.cin_pad = 2 * H;
    F.cout = kBigruFc1;
    F.K = 1;
    if ((rc = plan_layer(F)) != HIFICAR_OK) return rc;
    if ((rc = feature_alloc(h, pack_w32_elems(F, F.chunk16) * sizeof(float), &p)) != HIFICAR_OK) return rc;
    F.d_w32 = static_cast<float*>(p);
    if ((rc = feature_alloc(h, (size_t)F.cout_total * sizeof(float), &p)) != HIFICAR_OK) return rc;
    F.d_bias = static_cast<float*>(p);
    ConvLayer& Hh = ts->hh;
    Hh.name = "gru#hh";
    Hh.cin = Hh.cin_pad = H;
    Hh.cout = 3 * H;
    Hh.K = 1;
    if ((rc = plan_layer(Hh)) != HIFICAR_OK) return rc;
    for (int l = 0; l < 2; ++l)
        if ((rc = make_dgrad_layer(h, g->proj[l], ts->dg_proj[l], nullptr)) != HIFICAR_OK) return rc;
    if ((rc = make_dgrad_layer(h, F, ts->dg_fc1, nullptr)) != HIFICAR_OK) return rc;
    for (int l = 0; l < 2; ++l) {
        if ((rc = feature_alloc(h, (size_t)2 * 3 * (H / 8) * 2 * H * sizeof(float4), &p)) != HIFICAR_OK) return rc;
        ts->d_whht[l] = static_cast<float4*>(p);
    }
    if ((rc = wgrad_setup()) != HIFICAR_OK) return rc;
    HIP_TRY((bigru_train_attr<64, 1>()));
    HIP_TRY((bigru_train_attr<64, 2>()));
    HIP_TRY((bigru_train_attr<128, 1>()));
    HIP_TRY((bigru_train_attr<128, 2>()));
    HIP_TRY((bigru_train_attr<192, 1>()));
    HIP_TRY((bigru_train_attr<192, 2>()));
    HIP_TRY((bigru_train_attr<256, 1>()));
    HIP_TRY((bigru_train_attr<256, 2>()));
    return HIFICAR_OK;
}

extern "C" int hificar_bigru_grad_count(hificar_bigru* g) {
    return g && bigru_train_init(g) == HIFICAR_OK ? (int)g->train->tab.slots.size() : -1;
}

extern "C" int hificar_bigru_grad_info(hificar_bigru* g, int i, char* name96, int64_t* offset, int64_t* numel) {
    if (!g || !name96 || !offset || !numel) return fail(HIFICAR_E_INVALID, "hificar_bigru_grad_info: null argument");
    const int rc = bigru_train_init(g);
    return rc != HIFICAR_OK ? rc : feature_grad_info(g->train->tab, i, name96, offset, numel);
}

extern "C" int64_t hificar_bigru_grad_floats(hificar_bigru* g) {
    return g && bigru_train_init(g) == HIFICAR_OK ? g->train->tab.grad_total : -1;
}

// forward pack + bias of a one-tap layer, and its data-gradient pack, from a (cout, cin) weight in the master copy (as pack_jobs_for)
static int bigru_pack_layer(const ConvLayer& L, const ConvLayer* D, const float* w, const float* b, hipStream_t stream) {
    int rc;
    PackParams pp;
    fill_pack(pp, L, L.chunk16);
    pp.src = w;
    pp.dst = L.d_w32;
    pp.mode = 0;
    pp.cin = L.cin;
    pp.cout = L.cout;
    pp.K = L.K;
    pp.cin_pack = L.cin;
    pp.cout_pack = L.cout;
    if ((rc = launch_pack(pp, stream)) != HIFICAR_OK) return rc;
    PackParams pb = simple_pack(6, b, L.d_bias, (long long)L.n_phase * L.cout);
    pb.cout = L.cout;
    pb.cout_pad = L.cout_pad;
    if ((rc = launch_pack(pb, stream)) != HIFICAR_OK) return rc;
    if (D) {
        fill_pack(pp, *D, D->chunk16);
        pp.src = w;
        pp.dst = D->d_w32;
        pp.mode = 2;
        pp.cin = L.cin;
        pp.cout = L.cout;
        pp.K = L.K;
        pp.cin_pack = L.cout;
        pp.cout_pack = L.cin;
        if ((rc = launch_pack(pp, stream)) != HIFICAR_OK) return rc;
    }
    return HIFICAR_OK;
}

// Every float tensor of the state_dict (reference names and layouts; n of them, each exactly once) from DEVICE memory: copied into the
// handle's master copy and every derived form — the GEMM packs, W_hh and its transpose in the sweeps' orders, the eval path's folded fc1 —
// rebuilt on the device, on `stream`.  A list that is refused (feature_upload) leaves the handle exactly as it was.
extern "C" int hificar_bigru_set_parameters_device(hificar_bigru* g, const char* const* names, const float* const* data, int n, void* stream_) {
    if (!g || !names || !data) return fail(HIFICAR_E_INVALID, "hificar_bigru_set_parameters_device: null argument");
    int rc = bigru_train_init(g);
    if (rc != HIFICAR_OK) return rc;
    BigruTrain* ts = g->train;
    hificar_engine* h = &g->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    if ((rc = feature_upload(g->weights.expected, ts->tab, names, data, n, "hificar_bigru_set_parameters_device", stream)) != HIFICAR_OK) return rc;
    const int H = g->cfg.hidden_size, O = g->cfg.out_channels;
    float* const m = ts->tab.d_master;
    auto at = [&](const std::string& name) { return ts->tab.at(name); };
    for (int l = 0; l < 2; ++l) {
        const std::string b = "gru" + std::to_string(l + 1) + ".";
        if ((rc = bigru_pack_layer(g->proj[l], &ts->dg_proj[l], at(b + "weight_ih_l0"), at(b + "bias_ih_l0"), stream)) != HIFICAR_OK) return rc;
        hipLaunchKernelGGL(bigru_pack_whh_kernel, dim3(256), dim3(256), 0, stream, at(b + "weight_hh_l0"), reinterpret_cast<float*>(g->d_whh[l]),
                           reinterpret_cast<float*>(ts->d_whht[l]), H);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(g->d_bhh[l], at(b + "bias_hh_l0"), (size_t)6 * H * sizeof(float), hipMemcpyDeviceToDevice, stream));
    }
    if ((rc = bigru_pack_layer(ts->fc1_raw, &ts->dg_fc1, at("fc1.0.weight"), at("fc1.0.bias"), stream)) != HIFICAR_OK) return rc;
    hipLaunchKernelGGL(bigru_fold_fc1_kernel, dim3(kBigruFc1), dim3(256), 0, stream, at("fc1.0.weight"), at("fc1.0.bias"), at("bn.weight"), at("bn.bias"),
                       at("bn.running_mean"), at("bn.running_var"), m + ts->off_fold_w, m + ts->off_fold_b, 2 * H);
    HIP_TRY(hipGetLastError());
    if ((rc = bigru_pack_layer(g->fc1, nullptr, m + ts->off_fold_w, m + ts->off_fold_b, stream)) != HIFICAR_OK) return rc;
    HIP_TRY(hipMemcpyAsync(g->d_w2, at(bigru_fc2_name(g) + ".weight"), (size_t)O * kBigruFc1 * sizeof(float), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(g->d_b2, at(bigru_fc2_name(g) + ".bias"), (size_t)O * sizeof(float), hipMemcpyDeviceToDevice, stream));
    ts->have_params = true;
    return HIFICAR_OK;
}

// ------------------------------------------------------------------------------------------------
// tape and workspaces
// ------------------------------------------------------------------------------------------------
// feature_train_rows leaves at least 64 slack rows of 8H >= 512 floats behind a layer's gate values: room for this many frame counts
constexpr int kBigruRaggedMaxB = 32768;

struct BigruTape {
    BigruTapeHeader* hdr;
    float* x0;       // [rows][cin_pad] input rows
    float* y[2];     // [rows][2H] the layers' outputs (before dropout)
    float* gates[2]; // [rows][2][4H]
    float* f1;       // [rows][128] raw fc1
    float* stats;    // [3][128]
    float* out;      // (B, O, T)
    int* lens;       // [B] frame counts of a ragged forward (the header says whether they hold): in the slack rows behind the first layer's
                     // gate values, which no kernel reads or writes (the tape's size is that of a dense one); a tape-less forward: a piece of its own
    double* zstats;  // [B][mean, 1 / std] of a low-rate forward with zscore: in the slack rows behind the second layer's gate values, as lens
                     // (a tape-less forward keeps them in the workspace's gh, which only a backward pass uses: null here)
    size_t bytes;
};

// the slack rows behind a layer's gate values (64 rows of 8H >= 512 floats) hold this many utterances' statistics
constexpr int kBigruZscoreMaxB = 8192;

// The input of a low-rate step (hificar_bigru_forward_train_lowrate): Tl low-rate frames per sequence, T = factor Tl.  Tl = 0: the input is at
// the model's rate (hificar_bigru_forward_train[_ragged]).
struct BigruLow {
    int Tl = 0, factor = 1, zscore = 0;
};

// with_gates = false: what a forward alone needs (no per-step gate values): the tape-less form, laid out inside the workspace.
// Tl > 0: the input block holds the B Tl low-rate rows; everything behind it is the tape of B x T frames.
static BigruTape bigru_plan_tape(const hificar_bigru* g, int B, int T, void* base, bool with_gates = true, int Tl = 0) {
    const size_t rows = feature_train_rows(B, T), H = (size_t)g->cfg.hidden_size;
    Carver cv(base, 256);
    BigruTape t;
    t.hdr = cv.take<BigruTapeHeader>(256);
    t.x0 = cv.floats((Tl > 0 ? feature_train_rows(B, Tl) : rows) * g->cin_pad);
    for (int l = 0; l < 2; ++l) t.y[l] = cv.floats(rows * 2 * H);
    for (int l = 0; l < 2; ++l) t.gates[l] = with_gates ? cv.floats(rows * 8 * H) : nullptr;
    t.f1 = cv.floats(rows * kBigruFc1);
    t.stats = cv.floats(3 * kBigruFc1);
    t.out = cv.floats((size_t)B * T * g->cfg.out_channels);
    t.lens = with_gates ? reinterpret_cast<int*>(t.gates[0] + (base ? (size_t)B * T * 8 * H : 0)) : cv.take<int>((size_t)B * 4);
    t.zstats = nullptr;
    if (Tl > 0 && with_gates) t.zstats = reinterpret_cast<double*>(t.gates[1] + (base ? (size_t)B * T * 8 * H : 0));
    t.bytes = cv.bytes();
    return t;
}

struct BigruTrainWs {
    float* gx;      // [rows][6H]: forward: pre-gates; backward: gradient of W_ih x + b_ih
    float* gh;      // [rows][6H]: backward: gradient of W_hh h + b_hh
    float* a;       // [rows][2H]: dropout(y) (the next GEMM's input) / the gradient of a layer's output
    float* b;       // [rows][2H]: h of the step before
    float* dbn;     // [rows][128]
    float* dxr;     // [rows][cin_pad]
    float* partial; // weight-gradient partials
    float* colsum;  // bias-gradient partials
    float* head;    // fc2 partials [tiles][O * 128 + O]
    char* light;    // a forward without a tape keeps its rows here (bigru_plan_tape without the gate values)
    float* gxl;     // [low-rate rows][6H], a low-rate step at factor > 1 only: layer 1's pre-gates at the low rate / the adjoint interpolation of dgx
    size_t partial_elems, colsum_elems;
    size_t bytes;
};

// low.Tl > 0: the workspace of a low-rate step: that of B x T frames and, behind it, the [B Tl][6H] buffer (factor > 1)
static BigruTrainWs bigru_plan_train_ws(const hificar_bigru* g, int B, int T, void* base, const BigruLow& low = BigruLow()) {
    const size_t rows = feature_train_rows(B, T), H = (size_t)g->cfg.hidden_size;
    const int M = B * T;
    Carver cv(base, 256);
    BigruTrainWs w;
    w.gx = cv.floats(rows * 6 * H);
    w.gh = cv.floats(rows * 6 * H);
    w.a = cv.floats(rows * 2 * H);
    w.b = cv.floats(rows * 2 * H);
    w.dbn = cv.floats(rows * kBigruFc1);
    w.dxr = cv.floats(rows * g->cin_pad);
    w.partial_elems = w.colsum_elems = 0;
    if (g->train) {
        const hificar_engine* h = &g->eng;
        for (const ConvLayer* L : {&g->proj[0], &g->proj[1], (const ConvLayer*)&g->train->fc1_raw, (const ConvLayer*)&g->train->hh}) {
            w.partial_elems = std::max(w.partial_elems, wgrad_partial_elems(h, *L, 1, M));
            w.colsum_elems = std::max(w.colsum_elems, wgrad_colsum_elems(h, *L, 1, M));
        }
        if (low.Tl > 0) {  // layer 1's weight gradient runs over the B Tl low-rate rows (its row split is chosen by the row count)
            w.partial_elems = std::max(w.partial_elems, wgrad_partial_elems(h, g->proj[0], 1, B * low.Tl));
            w.colsum_elems = std::max(w.colsum_elems, wgrad_colsum_elems(h, g->proj[0], 1, B * low.Tl));
        }
    }
    w.partial = cv.floats(w.partial_elems);
    w.colsum = cv.floats(w.colsum_elems);
    const size_t tiles = (size_t)B * ((T + 63) / 64);
    w.head = cv.floats(tiles * (g->cfg.out_channels * (kBigruFc1 + 1)));
    w.light = cv.take<char>(bigru_plan_tape(g, B, T, nullptr, false, low.Tl).bytes);
    w.gxl = low.Tl > 0 && low.factor > 1 ? cv.floats(feature_train_rows(B, low.Tl) * 6 * H) : nullptr;
    w.bytes = cv.bytes();
    return w;
}

extern "C" size_t hificar_bigru_tape_bytes(const hificar_bigru* g, int B, int T) {
    if (!g || B < 1 || T < 1) return 0;
    return bigru_plan_tape(g, B, T, nullptr).bytes;
}

extern "C" size_t hificar_bigru_train_workspace_bytes(hificar_bigru* g, int B, int T) {
    if (!g || B < 1 || T < 1 || bigru_train_init(g) != HIFICAR_OK) return 0;
    return bigru_plan_train_ws(g, B, T, nullptr).bytes;
}

static int bigru_train_check(hificar_bigru* g, const char* what, int B, int T, void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes,
                             bool tape_optional = false) {
    if (!g) return fail(HIFICAR_E_INVALID, "%s: null handle", what);
    int rc = bigru_train_init(g);
    if (rc != HIFICAR_OK) return rc;
    if (!g->train->have_params) return fail(HIFICAR_E_STATE, "%s before hificar_bigru_set_parameters_device", what);
    if (B < 1 || T < 1 || B > 65535 || (long long)B * T > (1LL << 30) / 8) return fail(HIFICAR_E_INVALID, "%s: B=%d, T=%d out of range", what, B, T);
    if ((long long)B * T < 2) return fail(HIFICAR_E_INVALID, "%s: batch statistics need more than one frame (B * T = 1)", what);
    if ((!tape && !tape_optional) || reinterpret_cast<uintptr_t>(tape) % 256 || !workspace || reinterpret_cast<uintptr_t>(workspace) % 256)
        return fail(HIFICAR_E_INVALID, "%s: tape and workspace must be 256-byte aligned device pointers", what);
    const size_t tb = bigru_plan_tape(g, B, T, nullptr).bytes, wb = bigru_plan_train_ws(g, B, T, nullptr).bytes;
    if (tape && tape_bytes < tb) return fail(HIFICAR_E_WORKSPACE, "%s: tape too small: %zu < %zu", what, tape_bytes, tb);
    return check_workspace_size(what, workspace_bytes, wb);
}

static int bigru_gemm(hificar_engine* h, const ConvLayer& L, const float* x, float* y, int M, hipStream_t stream) {
    ConvIO io{};
    io.xs = reinterpret_cast<const char*>(x);
    io.y = y;
    const Ragged rg;
    return launch_conv1(h, L, 1, M, io, 0.f, rg, stream);
}

static int bigru_dropout(hificar_engine* h, const float* in, float* out, size_t n, const BigruTapeHeader* hdr, int site, hipStream_t stream) {
    ProfScope prof(h, stream, "bigru_dropout_kernel", 0.0, 8.0 * n);
    hipLaunchKernelGGL(bigru_dropout_kernel, dim3((unsigned)std::min<size_t>((n / 4 + 255) / 256, 4096)), dim3(256), 0, stream, in, out, (long long)n, hdr, site);
    HIP_TRY(hipGetLastError());
    return HIFICAR_OK;
}

static void bigru_head_params(const hificar_bigru* g, const BigruTape& tp, int B, int T, BigruHeadTrainParams& p) {
    const BigruTrain* ts = g->train;
    memset(&p, 0, sizeof(p));
    p.f1 = tp.f1;
    p.stats = tp.stats;
    p.gamma = ts->tab.at("bn.weight");
    p.beta = ts->tab.at("bn.bias");
    p.w2 = ts->tab.at(bigru_fc2_name(g) + ".weight");
    p.b2 = ts->tab.at(bigru_fc2_name(g) + ".bias");
    p.hdr = tp.hdr;
    p.lens = tp.lens;
    p.out_keep = tp.out;
    p.B = B;
    p.T = T;
    p.O = g->cfg.out_channels;
    p.use_tanh = g->cfg.use_tanh;
}

// The forward of train() mode: dropout with probability dropout_p behind each GRU layer and fc1 (masks: seed, offset — the caller's count of
// training forwards), batch norm on this batch's statistics, which come back in bn_batch_stats (mean | biased variance, 2 x 128 floats on the
// device).  Everything the backward pass needs stays in `tape` (hificar_bigru_tape_bytes), owned by the caller until hificar_bigru_backward ran.
// tape = NULL: the same arithmetic without a tape (no gate values are written; the rows live in the workspace): no backward pass can follow.
// lengths = null: the dense form.  Otherwise B frame counts on the device and their sum (checked by the caller): the ragged form.
static int bigru_forward_train_impl(hificar_bigru* g, const char* what, const float* x, const int* lengths, int valid, float* out, float* bn_batch_stats, int B,
                                    int T, float dropout_p, uint64_t seed, uint64_t offset, void* tape, void* workspace, void* stream_,
                                    const BigruLow& low = BigruLow()) {
    if (!x || !out || !bn_batch_stats) return fail(HIFICAR_E_INVALID, "%s: null tensor", what);
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) return fail(HIFICAR_E_INVALID, "%s: dropout_p=%g outside [0, 1)", what, (double)dropout_p);
    int rc;
    hificar_engine* h = &g->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    BigruTrain* ts = g->train;
    const BigruTrainWs ws = bigru_plan_train_ws(g, B, T, workspace, low);
    const BigruTape tp = tape ? bigru_plan_tape(g, B, T, tape, true, low.Tl) : bigru_plan_tape(g, B, T, ws.light, false, low.Tl);
    const int H = g->cfg.hidden_size, C = g->cfg.in_channels, O = g->cfg.out_channels, M = B * T;
    const int Tl = low.Tl, Ml = B * Tl;  // (a low-rate step: `lengths` are LOW-RATE frame counts, `valid` and the tape's counts are at the model's rate)
    hipLaunchKernelGGL(bigru_header_kernel, dim3(1), dim3(1), 0, stream, tp.hdr, (unsigned long long)seed, (unsigned long long)offset, dropout_p, B, T,
                       lengths ? valid : M, lengths ? 1 : 0, low.factor, Tl ? Tl : T, low.zscore);
    HIP_TRY(hipGetLastError());
    if (lengths && !Tl) HIP_TRY(hipMemcpyAsync(tp.lens, lengths, (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, stream));
    if (lengths && Tl) {
        hipLaunchKernelGGL(frontend_lengths_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, lengths, tp.lens, B, Tl, low.factor);
        HIP_TRY(hipGetLastError());
    }
    // the frames a ragged sweep does not write are operands of the GEMMs behind it (0 * NaN is NaN): zeros, written by this call
    auto zero_pad = [&](float* rows, int width) -> int {
        if (!lengths) return HIFICAR_OK;
        ProfScope prof(h, stream, "bigru_zero_pad_kernel", 0.0, 4.0 * (M - valid) * width);
        hipLaunchKernelGGL(bigru_zero_pad_kernel, dim3((unsigned)std::min<long long>(((long long)T * (width / 4) + 255) / 256, 8), (unsigned)B), dim3(256), 0,
                           stream, rows, width, tp.lens, T);
        HIP_TRY(hipGetLastError());
        return HIFICAR_OK;
    };
    if (Tl) {
        // the tape's input rows at the LOW rate (z-scored on the way): the interpolation commutes with the projection behind them, forwards
        // and backwards.  Padded low-rate rows — an operand of layer 1's dW_ih — are zeros written without reading x.
        double* const zstats = tape ? tp.zstats : reinterpret_cast<double*>(ws.gh);
        if (low.zscore) {
            ProfScope prof(h, stream, "frontend_stats_kernel", 0.0, 8.0 * Ml * C);
            hipLaunchKernelGGL(frontend_stats_kernel, dim3((unsigned)B), dim3(256), 0, stream, x, lengths, zstats, C, Tl);
            HIP_TRY(hipGetLastError());
        }
        ProfScope prof(h, stream, "frontend_rows_kernel", 0.0, 4.0 * Ml * (C + g->cin_pad));
        hipLaunchKernelGGL(frontend_rows_kernel<false>, dim3((unsigned)((Tl + 31) / 32), (unsigned)(g->cin_pad / 32), (unsigned)B), dim3(256), 0, stream, x, tp.x0,
                           static_cast<char*>(nullptr), lengths, low.zscore ? zstats : static_cast<const double*>(nullptr), C, g->cin_pad, Tl, 1);
        HIP_TRY(hipGetLastError());
    } else {
        {
            ProfScope prof(h, stream, "bigru_rows_kernel", 0.0, 4.0 * M * (C + g->cin_pad));
            hipLaunchKernelGGL(bigru_rows_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)(g->cin_pad / 32), (unsigned)B), dim3(256), 0, stream, x, tp.x0, C,
                               g->cin_pad, T);
            HIP_TRY(hipGetLastError());
        }
        if ((rc = zero_pad(tp.x0, g->cin_pad)) != HIFICAR_OK) return rc;
    }
    const int NS = bigru_tile_height(g, B);
    for (int l = 0; l < 2; ++l) {
        if (l == 0 && Tl) {  // layer 1's projection over the B Tl low-rate rows, its 6H-wide pre-gates interpolated
            if ((rc = bigru_gemm(h, g->proj[0], tp.x0, low.factor > 1 ? ws.gxl : ws.gx, Ml, stream)) != HIFICAR_OK) return rc;
            if (low.factor > 1) {
                const int N4 = 6 * H / 4;
                ProfScope prof(h, stream, "bigru_interp_gates_kernel", 3.0 * M * 6 * H, 4.0 * M * 6 * H * 3);
                hipLaunchKernelGGL(bigru_interp_gates_kernel, dim3((unsigned)(((long long)T * N4 + 255) / 256), 1, (unsigned)B), dim3(256), 0, stream, ws.gxl, ws.gx,
                                   lengths, N4, Tl, low.factor);
                HIP_TRY(hipGetLastError());
            }
        } else if ((rc = bigru_gemm(h, g->proj[l], l == 0 ? tp.x0 : ws.a, ws.gx, M, stream)) != HIFICAR_OK) return rc;
        if ((rc = zero_pad(tp.y[l], 2 * H)) != HIFICAR_OK) return rc;  // (the sweep writes the other rows: no order between the two)
        BigruRecParams p;
        p.g = ws.gx;
        p.w = g->d_whh[l];
        p.bhh = g->d_bhh[l];
        p.lengths = lengths ? tp.lens : nullptr;  // (the gate values of padded rows are never written and never read)
        p.y = tp.y[l];
        p.B = B;
        p.T = T;
        p.tape = tp.gates[l];
        {
            ProfScope prof(h, stream, "bigru_rec_kernel", 2.0 * M * 2 * 3 * H * H, 4.0 * M * 16 * H);
            const hipError_t e = tape ? HIFICAR_BIGRU_BY_SHAPE(bigru_rec_train_launch_one, H, NS, p, stream)
                                      : (NS == 1 ? bigru_rec_launch_h<1>(H, p, stream) : bigru_rec_launch_h<2>(H, p, stream));  // the inference sweep: same h
            if (e != hipSuccess) return fail(HIFICAR_E_HIP, "bigru_rec_kernel launch failed: %s", hipGetErrorString(e));
        }
        if ((rc = bigru_dropout(h, tp.y[l], ws.a, (size_t)M * 2 * H, tp.hdr, l == 0 ? kBigruSiteGru1 : kBigruSiteGru2, stream)) != HIFICAR_OK) return rc;
    }
    if ((rc = bigru_gemm(h, ts->fc1_raw, ws.a, tp.f1, M, stream)) != HIFICAR_OK) return rc;
    {
        ProfScope prof(h, stream, "bigru_bn_stats_kernel", 0.0, 8.0 * M * kBigruFc1);
        hipLaunchKernelGGL(bigru_bn_stats_kernel, dim3(kBigruFc1 / 32), dim3(1024), 0, stream, tp.f1, M, tp.hdr, tp.lens, tp.stats, bn_batch_stats);
        HIP_TRY(hipGetLastError());
    }
    {
        BigruHeadTrainParams p;
        bigru_head_params(g, tp, B, T, p);
        p.out = out;
        ProfScope prof(h, stream, "bigru_head_train_kernel", 2.0 * M * kBigruFc1 * O, 4.0 * M * (kBigruFc1 + 2 * O));
        hipLaunchKernelGGL(bigru_head_train_kernel, dim3((unsigned)((T + 63) / 64), (unsigned)B), dim3(256), 0, stream, p);
        HIP_TRY(hipGetLastError());
    }
    return HIFICAR_OK;
}

extern "C" int hificar_bigru_forward_train(hificar_bigru* g, const float* x, float* out, float* bn_batch_stats, int B, int T, float dropout_p, uint64_t seed,
                                           uint64_t offset, void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream_) {
    const int rc = bigru_train_check(g, "hificar_bigru_forward_train", B, T, tape, tape_bytes, workspace, workspace_bytes, true);
    if (rc != HIFICAR_OK) return rc;
    return bigru_forward_train_impl(g, "hificar_bigru_forward_train", x, nullptr, B * T, out, bn_batch_stats, B, T, dropout_p, seed, offset, tape, workspace,
                                    stream_);
}

// The same step on a ragged batch: sequence b has lengths[b] (0 .. T) frames of x (B, in_channels, T); what x holds past them is not used.
// Each sequence is swept over its own frames (the reverse direction starts at its own last one), the batch statistics are taken over the
// M = sum of lengths valid frames (M >= 2), out is zero past a length.  The dropout masks are those of the padded (B, T, C) tensor.  The tape
// keeps the lengths and M: hificar_bigru_backward on it ignores dout past a length, writes dx = 0 there and sums valid frames only.
// lengths: device int32[B]; lengths_host: the same values on the host (required: checked before anything is enqueued).
// All lengths = T: every result is bitwise that of hificar_bigru_forward_train.
extern "C" int hificar_bigru_forward_train_ragged(hificar_bigru* g, const float* x, const int32_t* lengths, const int32_t* lengths_host, float* out,
                                                  float* bn_batch_stats, int B, int T, float dropout_p, uint64_t seed, uint64_t offset, void* tape,
                                                  size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* what = "hificar_bigru_forward_train_ragged";
    const int rc = bigru_train_check(g, what, B, T, tape, tape_bytes, workspace, workspace_bytes, true);
    if (rc != HIFICAR_OK) return rc;
    if (!lengths || !lengths_host) return fail(HIFICAR_E_INVALID, "%s: lengths and lengths_host are both required", what);
    if (B > kBigruRaggedMaxB) return fail(HIFICAR_E_INVALID, "%s: B=%d above %d (what the tape's slack rows hold of lengths)", what, B, kBigruRaggedMaxB);
    long long valid = 0;
    for (int b = 0; b < B; ++b) {
        if (lengths_host[b] < 0 || lengths_host[b] > T) return fail(HIFICAR_E_INVALID, "%s: lengths[%d]=%d outside [0, %d]", what, b, (int)lengths_host[b], T);
        valid += lengths_host[b];
    }
    if (valid < 2) return fail(HIFICAR_E_INVALID, "%s: batch statistics need more than one valid frame (sum of lengths = %lld)", what, valid);
    return bigru_forward_train_impl(g, what, x, lengths, (int)valid, out, bn_batch_stats, B, T, dropout_p, seed, offset, tape, workspace, stream_);
}

// ------------------------------------------------------------------------------------------------
// Training on low-rate inputs: x (B, in_channels, Tl) at 1 / factor of the model's rate (and / or to be z-scored per utterance), the step that
// hificar_bigru_forward_train[_ragged] runs on the stretched input, T = factor Tl.  interp(X) W + b = interp(X W + b) holds under the chain
// rule too: with A the interpolation matrix, dW_ih = (A^T dGX)^T X_low, db_ih = column sums of A^T dGX (A's rows sum to one: those of dGX, to
// rounding), dX_low = (A^T dGX) W_ih.  So the tape keeps the B Tl low-rate rows, layer 1's projection, weight gradient and data gradient run
// over B Tl rows, and bigru_interp_gates_kernel / bigru_interp_gates_adj_kernel stand between them and the sweeps.
// ------------------------------------------------------------------------------------------------
extern "C" size_t hificar_bigru_tape_bytes_lowrate(const hificar_bigru* g, int B, int Tl, int factor) {
    if (!g || !lowrate_shape_ok(B, Tl, factor)) return 0;
    return bigru_plan_tape(g, B, Tl * factor, nullptr, true, Tl).bytes;  // (factor 1: the input block is that of B x Tl frames, the same bytes)
}

static BigruLow bigru_low(int Tl, int factor, int zscore) {
    BigruLow low;
    low.Tl = Tl;
    low.factor = factor;
    low.zscore = zscore ? 1 : 0;
    return low;
}

extern "C" size_t hificar_bigru_train_workspace_bytes_lowrate(hificar_bigru* g, int B, int Tl, int factor) {
    if (!g || !lowrate_shape_ok(B, Tl, factor) || bigru_train_init(g) != HIFICAR_OK) return 0;
    return bigru_plan_train_ws(g, B, Tl * factor, nullptr, bigru_low(Tl, factor, 0)).bytes;
}

// What both low-rate entry points check, in this order: the shape, the pointers' alignment and the sizes (on a handle without its training state:
// against the sizes known without the device, a lower bound) — everything that needs no device, so that a handle that was never finalized is
// told so last — then the state, then the sizes again with the weight-gradient partials the device's CU count decides.
static int bigru_lowrate_check(hificar_bigru* g, const char* what, int B, int Tl, int factor, int zscore, void* tape, size_t tape_bytes, void* workspace,
                               size_t workspace_bytes, bool tape_optional) {
    if (!g) return fail(HIFICAR_E_INVALID, "%s: null handle", what);
    if (factor < 1 || factor > HIFICAR_LOWRATE_MAX_FACTOR)
        return fail(HIFICAR_E_INVALID, "%s: factor=%d out of range (1 .. %d)", what, factor, HIFICAR_LOWRATE_MAX_FACTOR);
    if (!lowrate_shape_ok(B, Tl, factor)) return fail(HIFICAR_E_INVALID, "%s: B=%d, Tl=%d, factor=%d out of range", what, B, Tl, factor);
    if (zscore && B > kBigruZscoreMaxB)
        return fail(HIFICAR_E_INVALID, "%s: B=%d above %d with zscore (what the tape's slack rows hold of statistics)", what, B, kBigruZscoreMaxB);
    if ((!tape && !tape_optional) || reinterpret_cast<uintptr_t>(tape) % 256 || !workspace || reinterpret_cast<uintptr_t>(workspace) % 256)
        return fail(HIFICAR_E_INVALID, "%s: tape and workspace must be 256-byte aligned device pointers", what);
    const BigruLow low = bigru_low(Tl, factor, zscore);
    const size_t tb = bigru_plan_tape(g, B, Tl * factor, nullptr, true, Tl).bytes;
    for (int pass = 0; pass < 2; ++pass) {
        if (tape && tape_bytes < tb) return fail(HIFICAR_E_WORKSPACE, "%s: tape too small: %zu < %zu", what, tape_bytes, tb);
        const size_t wb = bigru_plan_train_ws(g, B, Tl * factor, nullptr, low).bytes;
        if (const int small = check_workspace_size(what, workspace_bytes, wb)) return small;
        if (pass == 1) break;
        if (!g->finalized) return fail(HIFICAR_E_STATE, "%s before hificar_bigru_finalize", what);
        const int rc = bigru_train_init(g);
        if (rc != HIFICAR_OK) return rc;
        if (!g->train->have_params) return fail(HIFICAR_E_STATE, "%s before hificar_bigru_set_parameters_device", what);
    }
    return HIFICAR_OK;
}

// lengths = NULL: the dense form (every sequence Tl low-rate frames).  Otherwise LOW-RATE frame counts: sequence b has factor * lengths[b]
// frames at the model's rate, and the step is hificar_bigru_forward_train_ragged's on the stretched batch: masks of the (B, T, C) tensors,
// batch statistics over M = factor * sum(lengths) >= 2 rows, out zero past factor * lengths[b].  Every sequence is interpolated by its own
// length (front_source / front_mix, clamped at its own last frame); padded low-rate frames of x are never read.  zscore: frontend_stats_kernel's
// utterance statistics, applied as constants.  tape = NULL: the forward-only form.  factor = 1 without zscore IS
// hificar_bigru_forward_train[_ragged]: the same launches, the same tape.
extern "C" int hificar_bigru_forward_train_lowrate(hificar_bigru* g, const float* x, const int32_t* lengths, const int32_t* lengths_host, float* out,
                                                   float* bn_batch_stats, int B, int Tl, int factor, int zscore, float dropout_p, uint64_t seed,
                                                   uint64_t offset, void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* what = "hificar_bigru_forward_train_lowrate";
    if (!g || !x || !out || !bn_batch_stats) return fail(HIFICAR_E_INVALID, "%s: null argument", what);
    if (factor < 1 || factor > HIFICAR_LOWRATE_MAX_FACTOR)
        return fail(HIFICAR_E_INVALID, "%s: factor=%d out of range (1 .. %d)", what, factor, HIFICAR_LOWRATE_MAX_FACTOR);
    if (!lowrate_shape_ok(B, Tl, factor)) return fail(HIFICAR_E_INVALID, "%s: B=%d, Tl=%d, factor=%d out of range", what, B, Tl, factor);
    if (!lengths != !lengths_host) return fail(HIFICAR_E_INVALID, "%s: lengths and lengths_host come together (both NULL: the dense form)", what);
    if (lengths && B > kBigruRaggedMaxB) return fail(HIFICAR_E_INVALID, "%s: B=%d above %d (what the tape's slack rows hold of lengths)", what, B, kBigruRaggedMaxB);
    long long valid = (long long)B * Tl;
    if (lengths_host) {
        valid = 0;
        for (int b = 0; b < B; ++b) {
            if (lengths_host[b] < 0 || lengths_host[b] > Tl)
                return fail(HIFICAR_E_INVALID, "%s: lengths[%d]=%d outside 0 .. Tl=%d", what, b, (int)lengths_host[b], Tl);
            valid += lengths_host[b];
        }
    }
    valid *= factor;
    if (valid < 2) return fail(HIFICAR_E_INVALID, "%s: batch statistics need more than one valid frame (factor * sum of lengths = %lld)", what, valid);
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) return fail(HIFICAR_E_INVALID, "%s: dropout_p=%g outside [0, 1)", what, (double)dropout_p);
    if (factor == 1 && !zscore) {
        // (the existing entry points on the same memory; their own checks repeat the ones above and come to the same verdicts)
        const size_t tb = hificar_bigru_tape_bytes(g, B, Tl);
        if ((tape && reinterpret_cast<uintptr_t>(tape) % 256) || !workspace || reinterpret_cast<uintptr_t>(workspace) % 256)
            return fail(HIFICAR_E_INVALID, "%s: tape and workspace must be 256-byte aligned device pointers", what);
        if (tape && tape_bytes < tb) return fail(HIFICAR_E_WORKSPACE, "%s: tape too small: %zu < %zu", what, tape_bytes, tb);
        if (workspace_bytes < bigru_plan_train_ws(g, B, Tl, nullptr).bytes) return fail(HIFICAR_E_WORKSPACE, "%s: workspace too small", what);
        if (!g->finalized) return fail(HIFICAR_E_STATE, "%s before hificar_bigru_finalize", what);
        return lengths ? hificar_bigru_forward_train_ragged(g, x, lengths, lengths_host, out, bn_batch_stats, B, Tl, dropout_p, seed, offset, tape, tape_bytes,
                                                            workspace, workspace_bytes, stream_)
                       : hificar_bigru_forward_train(g, x, out, bn_batch_stats, B, Tl, dropout_p, seed, offset, tape, tape_bytes, workspace, workspace_bytes,
                                                     stream_);
    }
    const int rc = bigru_lowrate_check(g, what, B, Tl, factor, zscore, tape, tape_bytes, workspace, workspace_bytes, true);
    if (rc != HIFICAR_OK) return rc;
    return bigru_forward_train_impl(g, what, x, lengths, (int)valid, out, bn_batch_stats, B, Tl * factor, dropout_p, seed, offset, tape, workspace, stream_,
                                    bigru_low(Tl, factor, zscore));
}

static int bigru_backward_impl(hificar_bigru* g, const float* dout, int B, int T, const void* tape, float* grads, float* dx, void* workspace, void* stream_,
                               const BigruLow& low);

// dout (B, O, T) -> the gradient of every parameter in `grads` (hificar_bigru_grad_floats floats, laid out as hificar_bigru_grad_info says;
// written, not accumulated) and, with dx non-null, of the input (B, in_channels, T).  The tape says whether its forward was ragged and with
// which lengths: then dout past a length is not read, dx is zero there and every gradient sums valid frames only.
extern "C" int hificar_bigru_backward(hificar_bigru* g, const float* dout, int B, int T, const void* tape, size_t tape_bytes, float* grads, float* dx,
                                      void* workspace, size_t workspace_bytes, void* stream_) {
    int rc = bigru_train_check(g, "hificar_bigru_backward", B, T, const_cast<void*>(tape), tape_bytes, workspace, workspace_bytes);
    if (rc != HIFICAR_OK) return rc;
    if (!dout || !grads) return fail(HIFICAR_E_INVALID, "hificar_bigru_backward: null tensor");
    return bigru_backward_impl(g, dout, B, T, tape, grads, dx, workspace, stream_, BigruLow());
}

// The backward pass of hificar_bigru_forward_train_lowrate: dout (B, O, factor Tl) -> grads as above and, with dx non-null, the input's
// gradient AT THE LOW RATE (B, in_channels, Tl), exactly zero on padded low-rate frames.  A separate entry point, not a tape that
// hificar_bigru_backward recognises: the tape's header lives on the device, so the host cannot read the layout out of it without a
// synchronising copy; B, Tl, factor and zscore are the forward's, as B and T are hificar_bigru_backward's.  A z-scored forward's dx is
// refused (the statistics' own derivative is not built).  factor = 1 without zscore IS hificar_bigru_backward.
extern "C" int hificar_bigru_backward_lowrate(hificar_bigru* g, const float* dout, int B, int Tl, int factor, int zscore, const void* tape, size_t tape_bytes,
                                              float* grads, float* dx, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* what = "hificar_bigru_backward_lowrate";
    if (!g || !dout || !grads) return fail(HIFICAR_E_INVALID, "%s: null argument", what);
    if (zscore && dx) return fail(HIFICAR_E_INVALID, "%s: dx of a z-scored forward is not built (the statistics are taken as constants)", what);
    if (factor == 1 && !zscore && lowrate_shape_ok(B, Tl, factor))
        return hificar_bigru_backward(g, dout, B, Tl, tape, tape_bytes, grads, dx, workspace, workspace_bytes, stream_);
    const int rc = bigru_lowrate_check(g, what, B, Tl, factor, zscore, const_cast<void*>(tape), tape_bytes, workspace, workspace_bytes, false);
    if (rc != HIFICAR_OK) return rc;
    return bigru_backward_impl(g, dout, B, Tl * factor, tape, grads, dx, workspace, stream_, bigru_low(Tl, factor, zscore));
}

static int bigru_backward_impl(hificar_bigru* g, const float* dout, int B, int T, const void* tape, float* grads, float* dx, void* workspace, void* stream_,
                               const BigruLow& low) {
    int rc;
    hificar_engine* h = &g->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    BigruTrain* ts = g->train;
    const BigruTape tp = bigru_plan_tape(g, B, T, const_cast<void*>(tape), true, low.Tl);
    const BigruTrainWs ws = bigru_plan_train_ws(g, B, T, workspace, low);
    const int H = g->cfg.hidden_size, C = g->cfg.in_channels, O = g->cfg.out_channels, M = B * T;
    auto G = [&](const std::string& name) { return grads + ts->tab.offset.at(name); };
    BwdWs bw = {};
    bw.partial = ws.partial;
    bw.colsum = ws.colsum;
    bw.partial_elems = ws.partial_elems;
    bw.colsum_elems = ws.colsum_elems;
    bw.accumulate = false;
    bw.defer = nullptr;
    {   // head: tanh', fc2
        BigruHeadTrainParams p;
        bigru_head_params(g, tp, B, T, p);
        const int tiles_t = (T + 63) / 64, tiles = B * tiles_t;
        p.dout = dout;
        p.dbn = ws.dbn;
        p.pw = ws.head;
        p.pb = ws.head + (size_t)tiles * O * kBigruFc1;
        {
            ProfScope prof(h, stream, "bigru_head_bwd_kernel", 4.0 * M * kBigruFc1 * O, 4.0 * M * (2 * kBigruFc1 + 2 * O));
            hipLaunchKernelGGL(bigru_head_bwd_kernel, dim3((unsigned)tiles_t, (unsigned)B), dim3(256), 0, stream, p);
            HIP_TRY(hipGetLastError());
        }
        ProfScope prof(h, stream, "bigru_colreduce_kernel", 0.0, 4.0 * tiles * O * (kBigruFc1 + 1));
        hipLaunchKernelGGL(bigru_colreduce_kernel, dim3((unsigned)((O * kBigruFc1 + 255) / 256)), dim3(256), 0, stream, p.pw, tiles, O * kBigruFc1,
                           G(bigru_fc2_name(g) + ".weight"));
        hipLaunchKernelGGL(bigru_colreduce_kernel, dim3(1), dim3(256), 0, stream, p.pb, tiles, O, G(bigru_fc2_name(g) + ".bias"));
        HIP_TRY(hipGetLastError());
    }
    {   // batch norm (batch statistics) and the dropout in front of it
        const float* gamma = ts->tab.at("bn.weight");
        ProfScope prof(h, stream, "bigru_bn_bwd_kernels", 0.0, 20.0 * M * kBigruFc1);
        hipLaunchKernelGGL(bigru_bn_bwd_sums_kernel, dim3(kBigruFc1 / 32), dim3(1024), 0, stream, tp.f1, ws.dbn, M, tp.hdr, tp.lens, tp.stats, G("bn.weight"),
                           G("bn.bias"));
        hipLaunchKernelGGL(bigru_bn_bwd_dx_kernel, dim3((unsigned)std::min<size_t>(((size_t)M * kBigruFc1 + 255) / 256, 4096)), dim3(256), 0, stream, tp.f1, ws.dbn,
                           M, tp.hdr, tp.lens, tp.stats, gamma, G("bn.weight"), G("bn.bias"));
        HIP_TRY(hipGetLastError());
    }
    // fc1: its input was dropout(y2)
    if ((rc = bigru_dropout(h, tp.y[1], ws.a, (size_t)M * 2 * H, tp.hdr, kBigruSiteGru2, stream)) != HIFICAR_OK) return rc;
    if ((rc = launch_wgrad(h, ts->fc1_raw, ws.dbn, kBigruFc1, ws.a, 2 * H, 1, M, G("fc1.0.weight"), bw, stream, G("fc1.0.bias"))) != HIFICAR_OK) return rc;
    if ((rc = bigru_gemm(h, ts->dg_fc1, ws.dbn, ws.a, M, stream)) != HIFICAR_OK) return rc;  // d(dropout(y2))
    const int NS = bigru_tile_height(g, B);
    for (int l = 1; l >= 0; --l) {
        const std::string b = "gru" + std::to_string(l + 1) + ".";
        if ((rc = bigru_dropout(h, ws.a, ws.a, (size_t)M * 2 * H, tp.hdr, l == 0 ? kBigruSiteGru1 : kBigruSiteGru2, stream)) != HIFICAR_OK) return rc;
        BigruRecBwdParams p;
        p.dy = ws.a;
        p.tape = tp.gates[l];
        p.y = tp.y[l];
        p.wt = ts->d_whht[l];
        p.dgx = ws.gx;
        p.dgh = ws.gh;
        p.B = B;
        p.T = T;
        p.hdr = tp.hdr;
        p.lens = tp.lens;
        {
            ProfScope prof(h, stream, "bigru_rec_bwd_kernel", 2.0 * M * 2 * 3 * H * H, 4.0 * M * 26 * H);
            const hipError_t e = HIFICAR_BIGRU_BY_SHAPE(bigru_rec_bwd_launch_one, H, NS, p, stream);
            if (e != hipSuccess) return fail(HIFICAR_E_HIP, "bigru_rec_bwd_kernel launch failed: %s", hipGetErrorString(e));
        }
        {
            const long long n4 = (long long)M * 2 * H / 4;
            ProfScope prof(h, stream, "bigru_hprev_kernel", 0.0, 16.0 * M * H);
            hipLaunchKernelGGL(bigru_hprev_kernel, dim3((unsigned)std::min<long long>((n4 + 255) / 256, 4096)), dim3(256), 0, stream, tp.y[l], ws.b, H, T, n4, tp.hdr, tp.lens);
            HIP_TRY(hipGetLastError());
        }
        for (int dir = 0; dir < 2; ++dir)  // dW_hh = dGH^T H_prev, db_hh: one direction's (3H, H) block at a time
            if ((rc = launch_wgrad(h, ts->hh, ws.gh + (size_t)dir * 3 * H, 6 * H, ws.b + (size_t)dir * H, 2 * H, 1, M,
                                   G(b + "weight_hh_l0") + (size_t)dir * 3 * H * H, bw, stream, G(b + "bias_hh_l0") + (size_t)dir * 3 * H)) != HIFICAR_OK)
                return rc;
        // dW_ih = dGX^T X, db_ih: the layer's input rows are the input itself / dropout(y1)
        const float* xin = tp.x0;
        if (l == 1) {
            if ((rc = bigru_dropout(h, tp.y[0], ws.b, (size_t)M * 2 * H, tp.hdr, kBigruSiteGru1, stream)) != HIFICAR_OK) return rc;
            xin = ws.b;
        }
        // a low-rate step's layer 1: the tape's rows are the B Tl low-rate ones, and dgx goes back to them through the interpolation's adjoint
        const float* dg = ws.gx;
        int Mx = M, Tx = T;
        if (l == 0 && low.Tl) {
            Tx = low.Tl;
            Mx = B * Tx;
            if (low.factor > 1) {
                const int N4 = 6 * H / 4;
                ProfScope prof(h, stream, "bigru_interp_gates_adj_kernel", 2.0 * M * 6 * H * 2, 4.0 * (2.0 * M + Mx) * 6 * H);
                hipLaunchKernelGGL(bigru_interp_gates_adj_kernel, dim3((unsigned)(((long long)Tx * N4 + 255) / 256), 1, (unsigned)B), dim3(256), 0, stream, ws.gx,
                                   ws.gxl, tp.hdr, tp.lens, N4, Tx, low.factor);
                HIP_TRY(hipGetLastError());
                dg = ws.gxl;
            }
        }
        if ((rc = launch_wgrad(h, g->proj[l], dg, 6 * H, xin, g->proj[l].cin_pad, 1, Mx, G(b + "weight_ih_l0"), bw, stream, G(b + "bias_ih_l0"))) != HIFICAR_OK)
            return rc;
        if (l == 1) {
            if ((rc = bigru_gemm(h, ts->dg_proj[1], ws.gx, ws.a, M, stream)) != HIFICAR_OK) return rc;  // d(dropout(y1))
        } else if (dx) {
            // (ragged: the padded rows of dgx are zeros, so those of dxr are sums of 0 * w: zeros, and bigru_unrows_kernel needs no mask)
            if ((rc = bigru_gemm(h, ts->dg_proj[0], dg, ws.dxr, Mx, stream)) != HIFICAR_OK) return rc;
            ProfScope prof(h, stream, "bigru_unrows_kernel", 0.0, 4.0 * Mx * (C + g->cin_pad));
            hipLaunchKernelGGL(bigru_unrows_kernel, dim3((unsigned)((Tx + 31) / 32), (unsigned)(g->cin_pad / 32), (unsigned)B), dim3(256), 0, stream, ws.dxr, dx, C,
                               g->cin_pad, Tx);
            HIP_TRY(hipGetLastError());
        }
    }
    return HIFICAR_OK;
}
