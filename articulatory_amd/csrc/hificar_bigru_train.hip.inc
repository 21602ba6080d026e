// Training of the BiGRU inversion model (the reference's step: articulatory/bin/train.py:241-383 through pytorch_models.py:45-72 in
// train() mode): device-resident parameters, the training-mode forward with its tape, and the backward pass.
//   forward   rows -> [proj GEMM -> recurrent sweep (keeps r, z, n, W_hn h + b_hn) -> dropout] x 2 -> raw fc1 GEMM -> batch statistics
//             -> dropout + batch norm + fc2 (+ tanh) in the head kernel
//   backward  head (tanh', dW_fc2, db_fc2) -> batch norm + dropout -> fc1 (dW, db, dY2) -> [dropout mask -> backward sweep -> dW_ih, db_ih,
//             dW_hh, db_hh, dX] x 2 -> dx
// The GEMMs are the conv engine's one-tap launches (forward and data gradients) and the weight-gradient kernels of hificar_train.hip.inc.
// Ragged batches (hificar_bigru_forward_train_ragged): every sequence is swept over its own frame count, the batch statistics and every
// gradient take the valid frames only; the GEMMs still run over all B T rows, and zeros in the padded rows of their operands mask them.
// Kernels: hificar_bigru_train_kernels.hip.h.

struct BigruTrain {
    struct Slot {
        std::string name;
        std::vector<int64_t> shape;
        int64_t offset, numel;
    };
    std::vector<Slot> slots;  // the trainable parameters in gradient-buffer order (reference names and layouts)
    std::map<std::string, int64_t> offset;  // name -> floats into the master copy (the trainable ones: = into the gradient buffer)
    int64_t grad_total = 0;    // floats of the gradient buffer
    int64_t master_total = 0;  // ... of the master copy: the parameters, bn.running_mean / running_var, the folded fc1 (eval form)
    int64_t off_fold_w = 0, off_fold_b = 0;
    float* d_master = nullptr;
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

static int bigru_alloc(hificar_engine* h, size_t bytes, void** out) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    h->allocs.push_back(p);
    HIP_TRY(hipMemset(p, 0, bytes));
    *out = p;
    return HIFICAR_OK;
}

static int bigru_train_build(hificar_bigru* g, BigruTrain* ts);

static int bigru_train_init(hificar_bigru* g) {
    if (g->train) return HIFICAR_OK;
    if (!g->finalized) return fail(HIFICAR_E_STATE, "BiGRU training entry points need hificar_bigru_finalize first");
    // a failed set-up (out of device memory, in practice) is final for this handle: what it allocated stays on the engine's allocation list until
    // destroy, so another attempt per entry point would only grow that list
    if (g->train_failed != HIFICAR_OK) return fail(g->train_failed, "the BiGRU training state could not be set up on this handle earlier; destroy it and make a new one");
    std::unique_ptr<BigruTrain> ts(new BigruTrain());
    const int rc = bigru_train_build(g, ts.get());
    if (rc != HIFICAR_OK) {
        g->train_failed = rc;
        return rc;  // nothing half-built stays behind
    }
    g->train = ts.release();
    return HIFICAR_OK;
}

static int bigru_train_build(hificar_bigru* g, BigruTrain* ts) {
    hificar_engine* h = &g->eng;
    const int H = g->cfg.hidden_size;
    int64_t total = 0;
    auto add = [&](const std::string& name, bool trainable) {
        const std::vector<int64_t>& shape = g->expected.at(name);
        int64_t n = 1;
        for (auto v : shape) n *= v;
        ts->offset[name] = total;
        if (trainable) ts->slots.push_back({name, shape, total, n});
        total += (n + 3) & ~(int64_t)3;
    };
    // a layer's forward and reverse tensors of one kind lie back to back: (6H, Cin) / (6H) / 2 x (3H, H) blocks, as the GEMMs see them
    for (int l = 1; l <= 2; ++l) {
        const std::string b = "gru" + std::to_string(l) + ".";
        for (const char* kind : {"weight_ih_l0", "bias_ih_l0", "weight_hh_l0", "bias_hh_l0"})
            for (const char* sfx : {"", "_reverse"}) add(b + kind + sfx, true);
    }
    for (const char* n : {"fc1.0.weight", "fc1.0.bias", "bn.weight", "bn.bias"}) add(n, true);
    add(bigru_fc2_name(g) + ".weight", true);
    add(bigru_fc2_name(g) + ".bias", true);
    ts->grad_total = total;
    add("bn.running_mean", false);
    add("bn.running_var", false);
    ts->off_fold_w = total;
    total += (int64_t)kBigruFc1 * 2 * H;
    ts->off_fold_b = total;
    total += kBigruFc1;
    ts->master_total = total;
    int rc;
    void* p = nullptr;
    if ((rc = bigru_alloc(h, (size_t)total * sizeof(float), &p)) != HIFICAR_OK) return rc;
    ts->d_master = static_cast<float*>(p);

    ConvLayer& F = ts->fc1_raw;
    F.name = "fc1#raw";
    F.cin = F.cin_pad = 2 * H;
    F.cout = kBigruFc1;
    F.K = 1;
    if ((rc = plan_layer(F)) != HIFICAR_OK) return rc;
    if ((rc = bigru_alloc(h, pack_w32_elems(F, F.chunk16) * sizeof(float), &p)) != HIFICAR_OK) return rc;
    F.d_w32 = static_cast<float*>(p);
    if ((rc = bigru_alloc(h, (size_t)F.cout_total * sizeof(float), &p)) != HIFICAR_OK) return rc;
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
        if ((rc = bigru_alloc(h, (size_t)2 * 3 * (H / 8) * 2 * H * sizeof(float4), &p)) != HIFICAR_OK) return rc;
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
    if (!g || bigru_train_init(g) != HIFICAR_OK) return -1;
    return (int)g->train->slots.size();
}

extern "C" int hificar_bigru_grad_info(hificar_bigru* g, int i, char* name96, int64_t* offset, int64_t* numel) {
    if (!g || !name96 || !offset || !numel) return fail(HIFICAR_E_INVALID, "hificar_bigru_grad_info: null argument");
    int rc = bigru_train_init(g);
    if (rc != HIFICAR_OK) return rc;
    if (i < 0 || i >= (int)g->train->slots.size()) return fail(HIFICAR_E_INVALID, "gradient index %d out of range", i);
    const BigruTrain::Slot& s = g->train->slots[(size_t)i];
    snprintf(name96, 96, "%s", s.name.c_str());
    *offset = s.offset;
    *numel = s.numel;
    return HIFICAR_OK;
}

extern "C" int64_t hificar_bigru_grad_floats(hificar_bigru* g) {
    if (!g || bigru_train_init(g) != HIFICAR_OK) return -1;
    return g->train->grad_total;
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
// rebuilt on the device, on `stream`.
extern "C" int hificar_bigru_set_parameters_device(hificar_bigru* g, const char* const* names, const float* const* data, int n, void* stream_) {
    if (!g || !names || !data) return fail(HIFICAR_E_INVALID, "hificar_bigru_set_parameters_device: null argument");
    int rc = bigru_train_init(g);
    if (rc != HIFICAR_OK) return rc;
    BigruTrain* ts = g->train;
    hificar_engine* h = &g->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    if (n != (int)g->expected.size()) return fail(HIFICAR_E_INVALID, "hificar_bigru_set_parameters_device: %d tensors, the model has %zu", n, g->expected.size());
    std::set<std::string> seen;
    for (int i = 0; i < n; ++i) {
        if (!names[i] || !data[i]) return fail(HIFICAR_E_INVALID, "hificar_bigru_set_parameters_device: null entry %d", i);
        auto it = g->expected.find(names[i]);
        if (it == g->expected.end()) return fail(HIFICAR_E_INVALID, "unexpected tensor name '%s' for this configuration", names[i]);
        if (!seen.insert(names[i]).second) return fail(HIFICAR_E_INVALID, "tensor '%s' given twice", names[i]);
        size_t numel = 1;
        for (auto v : it->second) numel *= (size_t)v;
        HIP_TRY(hipMemcpyAsync(ts->d_master + ts->offset.at(names[i]), data[i], numel * sizeof(float), hipMemcpyDeviceToDevice, stream));
    }
    const int H = g->cfg.hidden_size, O = g->cfg.out_channels;
    float* const m = ts->d_master;
    auto at = [&](const std::string& name) { return m + ts->offset.at(name); };
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
static size_t bigru_train_rows(int B, int T) { return round_up_sz((size_t)B * (size_t)T + 64, 256); }  // slack behind the last row for whole GEMM tiles

// bigru_train_rows leaves at least 64 slack rows of 8H >= 512 floats behind a layer's gate values: room for this many frame counts
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
    size_t bytes;
};

// with_gates = false: what a forward alone needs (no per-step gate values): the tape-less form, laid out inside the workspace
static BigruTape bigru_plan_tape(const hificar_bigru* g, int B, int T, void* base, bool with_gates = true) {
    const size_t rows = bigru_train_rows(B, T), H = (size_t)g->cfg.hidden_size;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? static_cast<char*>(base) + off : nullptr;
        off += round_up_sz(bytes, 256);
        return p;
    };
    BigruTape t;
    t.hdr = reinterpret_cast<BigruTapeHeader*>(take(256));
    t.x0 = reinterpret_cast<float*>(take(rows * g->cin_pad * 4));
    for (int l = 0; l < 2; ++l) t.y[l] = reinterpret_cast<float*>(take(rows * 2 * H * 4));
    for (int l = 0; l < 2; ++l) t.gates[l] = with_gates ? reinterpret_cast<float*>(take(rows * 8 * H * 4)) : nullptr;
    t.f1 = reinterpret_cast<float*>(take(rows * kBigruFc1 * 4));
    t.stats = reinterpret_cast<float*>(take(3 * kBigruFc1 * 4));
    t.out = reinterpret_cast<float*>(take((size_t)B * T * g->cfg.out_channels * 4));
    t.lens = with_gates ? reinterpret_cast<int*>(t.gates[0] + (base ? (size_t)B * T * 8 * H : 0)) : reinterpret_cast<int*>(take((size_t)B * 4));
    t.bytes = off;
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
    size_t partial_elems, colsum_elems;
    size_t bytes;
};

static BigruTrainWs bigru_plan_train_ws(const hificar_bigru* g, int B, int T, void* base) {
    const size_t rows = bigru_train_rows(B, T), H = (size_t)g->cfg.hidden_size;
    const int M = B * T;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? static_cast<char*>(base) + off : nullptr;
        off += round_up_sz(bytes, 256);
        return reinterpret_cast<float*>(p);
    };
    BigruTrainWs w;
    w.gx = take(rows * 6 * H * 4);
    w.gh = take(rows * 6 * H * 4);
    w.a = take(rows * 2 * H * 4);
    w.b = take(rows * 2 * H * 4);
    w.dbn = take(rows * kBigruFc1 * 4);
    w.dxr = take(rows * g->cin_pad * 4);
    w.partial_elems = w.colsum_elems = 0;
    if (g->train) {
        const hificar_engine* h = &g->eng;
        for (const ConvLayer* L : {&g->proj[0], &g->proj[1], (const ConvLayer*)&g->train->fc1_raw, (const ConvLayer*)&g->train->hh}) {
            w.partial_elems = std::max(w.partial_elems, wgrad_partial_elems(h, *L, 1, M));
            w.colsum_elems = std::max(w.colsum_elems, wgrad_colsum_elems(h, *L, 1, M));
        }
    }
    w.partial = take(w.partial_elems * 4);
    w.colsum = take(w.colsum_elems * 4);
    const size_t tiles = (size_t)B * ((T + 63) / 64);
    w.head = take(tiles * (g->cfg.out_channels * (kBigruFc1 + 1)) * 4);
    w.light = reinterpret_cast<char*>(take(bigru_plan_tape(g, B, T, nullptr, false).bytes));
    w.bytes = off;
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
    if (workspace_bytes < wb) return fail(HIFICAR_E_WORKSPACE, "%s: workspace too small: %zu < %zu", what, workspace_bytes, wb);
    return HIFICAR_OK;
}

static int bigru_gemm(hificar_engine* h, const ConvLayer& L, const float* x, float* y, int M, hipStream_t stream) {
    const ConvLayer* ls[1] = {&L};
    ConvIO io[1];
    io[0] = ConvIO();
    io[0].xs = reinterpret_cast<const char*>(x);
    io[0].y = y;
    const Ragged rg;
    return launch_conv(h, ls, 1, 1, M, io, 0.f, rg, stream);
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
    p.gamma = ts->d_master + ts->offset.at("bn.weight");
    p.beta = ts->d_master + ts->offset.at("bn.bias");
    p.w2 = ts->d_master + ts->offset.at(bigru_fc2_name(g) + ".weight");
    p.b2 = ts->d_master + ts->offset.at(bigru_fc2_name(g) + ".bias");
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
                                    int T, float dropout_p, uint64_t seed, uint64_t offset, void* tape, void* workspace, void* stream_) {
    if (!x || !out || !bn_batch_stats) return fail(HIFICAR_E_INVALID, "%s: null tensor", what);
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) return fail(HIFICAR_E_INVALID, "%s: dropout_p=%g outside [0, 1)", what, (double)dropout_p);
    int rc;
    hificar_engine* h = &g->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    BigruTrain* ts = g->train;
    const BigruTrainWs ws = bigru_plan_train_ws(g, B, T, workspace);
    const BigruTape tp = tape ? bigru_plan_tape(g, B, T, tape) : bigru_plan_tape(g, B, T, ws.light, false);
    const int H = g->cfg.hidden_size, C = g->cfg.in_channels, O = g->cfg.out_channels, M = B * T;
    hipLaunchKernelGGL(bigru_header_kernel, dim3(1), dim3(1), 0, stream, tp.hdr, (unsigned long long)seed, (unsigned long long)offset, dropout_p, B, T,
                       lengths ? valid : M, lengths ? 1 : 0);
    HIP_TRY(hipGetLastError());
    if (lengths) HIP_TRY(hipMemcpyAsync(tp.lens, lengths, (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, stream));
    // the frames a ragged sweep does not write are operands of the GEMMs behind it (0 * NaN is NaN): zeros, written by this call
    auto zero_pad = [&](float* rows, int width) -> int {
        if (!lengths) return HIFICAR_OK;
        ProfScope prof(h, stream, "bigru_zero_pad_kernel", 0.0, 4.0 * (M - valid) * width);
        hipLaunchKernelGGL(bigru_zero_pad_kernel, dim3((unsigned)std::min<long long>(((long long)T * (width / 4) + 255) / 256, 8), (unsigned)B), dim3(256), 0,
                           stream, rows, width, tp.lens, T);
        HIP_TRY(hipGetLastError());
        return HIFICAR_OK;
    };
    {
        ProfScope prof(h, stream, "bigru_rows_kernel", 0.0, 4.0 * M * (C + g->cin_pad));
        hipLaunchKernelGGL(bigru_rows_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)(g->cin_pad / 32), (unsigned)B), dim3(256), 0, stream, x, tp.x0, C,
                           g->cin_pad, T);
        HIP_TRY(hipGetLastError());
    }
    if ((rc = zero_pad(tp.x0, g->cin_pad)) != HIFICAR_OK) return rc;
    const int NS = bigru_tile_height(g, B);
    for (int l = 0; l < 2; ++l) {
        if ((rc = bigru_gemm(h, g->proj[l], l == 0 ? tp.x0 : ws.a, ws.gx, M, stream)) != HIFICAR_OK) return rc;
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

// dout (B, O, T) -> the gradient of every parameter in `grads` (hificar_bigru_grad_floats floats, laid out as hificar_bigru_grad_info says;
// written, not accumulated) and, with dx non-null, of the input (B, in_channels, T).  The tape says whether its forward was ragged and with
// which lengths: then dout past a length is not read, dx is zero there and every gradient sums valid frames only.
extern "C" int hificar_bigru_backward(hificar_bigru* g, const float* dout, int B, int T, const void* tape, size_t tape_bytes, float* grads, float* dx,
                                      void* workspace, size_t workspace_bytes, void* stream_) {
    int rc = bigru_train_check(g, "hificar_bigru_backward", B, T, const_cast<void*>(tape), tape_bytes, workspace, workspace_bytes);
    if (rc != HIFICAR_OK) return rc;
    if (!dout || !grads) return fail(HIFICAR_E_INVALID, "hificar_bigru_backward: null tensor");
    hificar_engine* h = &g->eng;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    BigruTrain* ts = g->train;
    const BigruTape tp = bigru_plan_tape(g, B, T, const_cast<void*>(tape));
    const BigruTrainWs ws = bigru_plan_train_ws(g, B, T, workspace);
    const int H = g->cfg.hidden_size, C = g->cfg.in_channels, O = g->cfg.out_channels, M = B * T;
    auto G = [&](const std::string& name) { return grads + ts->offset.at(name); };
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
        const float* gamma = ts->d_master + ts->offset.at("bn.weight");
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
        if ((rc = launch_wgrad(h, g->proj[l], ws.gx, 6 * H, xin, g->proj[l].cin_pad, 1, M, G(b + "weight_ih_l0"), bw, stream, G(b + "bias_ih_l0"))) != HIFICAR_OK)
            return rc;
        if (l == 1) {
            if ((rc = bigru_gemm(h, ts->dg_proj[1], ws.gx, ws.a, M, stream)) != HIFICAR_OK) return rc;  // d(dropout(y1))
        } else if (dx) {
            // (ragged: the padded rows of dgx are zeros, so those of dxr are sums of 0 * w: zeros, and bigru_unrows_kernel needs no mask)
            if ((rc = bigru_gemm(h, ts->dg_proj[0], ws.gx, ws.dxr, M, stream)) != HIFICAR_OK) return rc;
            ProfScope prof(h, stream, "bigru_unrows_kernel", 0.0, 4.0 * M * (C + g->cin_pad));
            hipLaunchKernelGGL(bigru_unrows_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)(g->cin_pad / 32), (unsigned)B), dim3(256), 0, stream, ws.dxr, dx, C,
                               g->cin_pad, T);
            HIP_TRY(hipGetLastError());
        }
    }
    return HIFICAR_OK;
}
