// Training support of libhificar (included at the end of hificar.hip): device-resident weights, the forward tape and the generator's
// backward pass.  Reference: the generator half of articulatory/bin/train.py:241-440 (PyTorch autograd through
// articulatory/models/hifigan.py:198-239).  Kernels: hificar_backward.hip.h.  Exact-fp32 arithmetic only.

// The raw parameters of one engine (the generator's TrainState, the discriminators' hificar_disc) and their batched hand-over
// (raw_set_parameters): the folded master copy in the gradient layout, the static table of every pack (sources inside the master copy) and
// the per-call table of fold / copy jobs (re-sent when a pointer moves).  Gradient buckets (data-parallel training: a bucket's gradients
// are complete, and can be all-reduced, while the rest of the backward pass still runs): every folded slot's bucket is fixed when the
// slot is added, and the ParamJob table is ordered by bucket.
struct RawParamSet {
    struct Slot {
        std::string name;
        std::vector<int64_t> shape;
        int64_t offset, numel;
        int bucket;
    };
    std::vector<Slot> slots;           // folded parameters in master-copy (= folded gradient buffer) order
    std::map<std::string, int> index;  // name -> slot
    int64_t total = 0;                 // floats of the master copy
    int n_buckets = 0;
    float* d_folded = nullptr;
    PackParams* d_pack_jobs = nullptr;
    int* d_pack_start = nullptr;
    int n_pack_jobs = 0, n_pack_wgs = 0;
    ParamJob* d_param_jobs = nullptr;
    int* d_param_start = nullptr;
    ParamJob* pin_param_jobs = nullptr;  // pinned mirrors
    int* pin_param_start = nullptr;
    std::vector<ParamJob> param_jobs;
    std::vector<std::string> raw_names;
    int n_param_wgs = 0;
    int64_t raw_total = 0;
    bool have_params = false;
    std::vector<int> job_slot;        // [job] its slot (slots stably sorted by bucket)
    std::vector<int> bucket_job_lo;   // [bucket] first job; bucket_job_lo[n_buckets] = number of jobs
    std::vector<int> raw_bucket;      // [raw parameter of the last hand-over] its bucket
    hificar_bucket_fn bucket_fn = nullptr;
    void* bucket_user = nullptr;

    RawParamSet() = default;
    RawParamSet(const RawParamSet&) = delete;
    RawParamSet& operator=(const RawParamSet&) = delete;
    ~RawParamSet() {
        if (pin_param_jobs) (void)hipHostFree(pin_param_jobs);
        if (pin_param_start) (void)hipHostFree(pin_param_start);
    }
    void add(const std::string& name, const std::vector<int64_t>& shape, int bucket) {
        int64_t n = 1;
        for (auto v : shape) n *= v;
        index[name] = (int)slots.size();
        slots.push_back({name, shape, total, n, bucket});
        total += (n + 3) & ~(int64_t)3;  // 16-byte aligned slots
    }
    int64_t offset(const std::string& name) const { return slots[(size_t)index.at(name)].offset; }
};

struct TrainState {
    // data-gradient layers (a Conv1d each) of every forward conv, in the forward lists' order
    ConvLayer dg_input;
    std::vector<ConvLayer> dg_ups, dg_c1, dg_c2;
    std::vector<ConvLayer> dg_gb;  // GBlockGenerator: [block][c1a, c1b, res, c2a, c2b]
    int up_jmin[HIFICAR_MAX_STAGES] = {};
    std::map<std::string, std::pair<ConvLayer*, ConvLayer*>> by_name;  // "input_conv" -> (forward layer, its dgrad layer)
    // folded parameters in the order of hificar_handle::expected (sorted by name).  Bucket b < n_stages: the ResBlocks of stage
    // n_stages - 1 - b (+ the output conv and the phoneme head in bucket 0); bucket n_stages ("front"): input conv, upsamplers,
    // PastFCEncoder, conditioning tensors (gen_bucket_of)
    RawParamSet raw;
};

// number of gradient buckets of the generator: one per stage (HiFi-GAN) / per GBlock, last first, + the "front" bucket
static int gen_bucket_count(const hificar_handle* h) { return (h->arch == 1 ? (int)h->gb.size() : h->cfg.n_stages) + 1; }

static int gen_bucket_of(const hificar_handle* h, const std::string& folded_name) {
    if (h->arch == 1) {  // GBlockGenerator: bucket b < n = GBlock n - 1 - b (+ the output conv in bucket 0); bucket n: input conv, PastFCEncoder, speaker tensors
        const int n = (int)h->gb.size();
        if (folded_name.rfind("resamples.", 0) == 0) return n - 1 - atoi(folded_name.c_str() + 10);
        return folded_name.rfind("output_conv.", 0) == 0 ? 0 : n;
    }
    const int ns = h->cfg.n_stages;
    if (folded_name.rfind("blocks.", 0) == 0) return ns - 1 - atoi(folded_name.c_str() + 7) / h->cfg.n_blocks;
    if (folded_name.rfind("output_conv.", 0) == 0 || folded_name.rfind("ph_fc.", 0) == 0) return 0;
    return ns;
}

static TrainState* train_state(hificar_handle* h) { return static_cast<TrainState*>(h->train); }

static size_t pack_w32_elems(const ConvLayer& L, int chunk) {
    const int nc16 = chunk / 16, nchunk = L.cin_pad / chunk;
    return ((size_t)L.n_blocks32 * nchunk * L.ntaps * nc16 * 2 + 4 * nc16) * 256;
}

static int make_dgrad_layer(hificar_engine* h, const ConvLayer& L, ConvLayer& D, int* jmin_out) {
    D = ConvLayer();
    D.name = L.name + "#dgrad";
    D.transposed = false;
    D.has_bias = false;
    D.cout = L.cin;
    if (!L.transposed) {
        D.cin = L.cout;
        D.cin_pad = L.cout_pad;
        D.K = L.K;
        D.dilation = L.dilation;
        D.padding = (L.K - 1) * L.dilation - L.padding;
    } else {
        // da[ci, i] = sum_{r, co, j} W[ci, co, r + s j + p] dy_v[i + j, (r, co)]: a Conv1d over the phase-major virtual channels of dy
        const int s = L.stride, p = L.padding;
        auto fdiv = [](int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); };
        const int jmin = fdiv(-p, s), jmax = fdiv(L.K - 1 - p, s);
        D.cin = D.cin_pad = L.cout_total;
        D.K = jmax - jmin + 1;
        D.dilation = 1;
        D.padding = -jmin;
        if (jmin_out) *jmin_out = jmin;
    }
    int rc = plan_layer(D);
    if (rc != HIFICAR_OK) return rc;
    std::vector<float> zeros((size_t)D.cout_total, 0.f);
    if ((rc = upload(h, zeros, &D.d_bias)) != HIFICAR_OK) return rc;
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, pack_w32_elems(D, D.chunk16) * sizeof(float)));
    h->allocs.push_back(p);
    HIP_TRY(hipMemset(p, 0, pack_w32_elems(D, D.chunk16) * sizeof(float)));
    D.d_w32 = static_cast<float*>(p);
    return HIFICAR_OK;
}

static int wgrad_setup() {
#define HIFICAR_WGT_LDS1(NT, EX, R) \
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_taps_kernel<NT, EX, R>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024))
#define HIFICAR_WGT_LDS(NT, EX)      \
    HIFICAR_WGT_LDS1(NT, EX, 32);    \
    HIFICAR_WGT_LDS1(NT, EX, 64);    \
    HIFICAR_WGT_LDS1((NT <= 7 ? NT : 7), EX, 128)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_gemm_kernel<2, 64>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_gemm_kernel<4, 32>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_bf16x3_kernel<2, 64>), hipFuncAttributeMaxDynamicSharedMemorySize, wgrad_bf16x3_lds<2, 64>()));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_bf16x3_kernel<4, 32>), hipFuncAttributeMaxDynamicSharedMemorySize, wgrad_bf16x3_lds<4, 32>()));
    HIFICAR_WGT_LDS(1, true);
    HIFICAR_WGT_LDS(2, true);
    HIFICAR_WGT_LDS(3, true);
    HIFICAR_WGT_LDS(7, true);
    HIFICAR_WGT_LDS(11, true);
    HIFICAR_WGT_LDS(7, false);
    HIFICAR_WGT_LDS(11, false);
#undef HIFICAR_WGT_LDS
    return HIFICAR_OK;
}

static void train_free_impl(hificar_handle* h) {
    delete train_state(h);
    h->train = nullptr;
}

static int train_init(hificar_handle* h) {
    if (h->train) return HIFICAR_OK;
    if (!h->finalized) return fail(HIFICAR_E_STATE, "training entry points need hificar_finalize first");
    if (h->cfg.use_ph_loss && h->cfg.num_ph > 256) return fail(HIFICAR_E_INVALID, "use_ph_loss training: num_ph <= 256 (got %d)", h->cfg.num_ph);
    if (h->cfg.use_ph && h->cfg.ph_emb_size > 256)
        return fail(HIFICAR_E_INVALID, "use_ph training: ph_emb_size <= 256 (got %d)", h->cfg.ph_emb_size);
    TrainState* ts = new TrainState();
    h->train = ts;
    h->training = true;
    h->train_free = train_free_impl;
    int rc;
    if ((rc = make_dgrad_layer(h, h->input_conv, ts->dg_input, nullptr)) != HIFICAR_OK) return rc;
    ts->by_name["input_conv"] = {&h->input_conv, &ts->dg_input};
    ts->dg_ups.resize(h->ups.size());
    ts->dg_c1.resize(h->convs1.size());
    ts->dg_c2.resize(h->convs2.size());
    for (size_t i = 0; i < h->ups.size(); ++i) {
        if ((rc = make_dgrad_layer(h, h->ups[i], ts->dg_ups[i], &ts->up_jmin[i])) != HIFICAR_OK) return rc;
        ts->by_name[h->ups[i].name] = {&h->ups[i], &ts->dg_ups[i]};
    }
    for (size_t i = 0; i < h->convs1.size(); ++i) {
        if ((rc = make_dgrad_layer(h, h->convs1[i], ts->dg_c1[i], nullptr)) != HIFICAR_OK) return rc;
        ts->by_name[h->convs1[i].name] = {&h->convs1[i], &ts->dg_c1[i]};
        if (i < h->convs2.size()) {  // (no convs2 with use_additional_convs = false)
            if ((rc = make_dgrad_layer(h, h->convs2[i], ts->dg_c2[i], nullptr)) != HIFICAR_OK) return rc;
            ts->by_name[h->convs2[i].name] = {&h->convs2[i], &ts->dg_c2[i]};
        }
    }
    ts->dg_gb.resize(h->gb.size() * 5);
    for (size_t i = 0; i < h->gb.size(); ++i) {
        ConvLayer* fw[5] = {&h->gb[i].c1a, &h->gb[i].c1b, &h->gb[i].res, &h->gb[i].c2a, &h->gb[i].c2b};
        for (int q = 0; q < 5; ++q) {
            if ((rc = make_dgrad_layer(h, *fw[q], ts->dg_gb[i * 5 + q], nullptr)) != HIFICAR_OK) return rc;
            ts->by_name[fw[q]->name] = {fw[q], &ts->dg_gb[i * 5 + q]};
        }
    }
    for (auto& kv : h->weights.expected) ts->raw.add(kv.first, kv.second, gen_bucket_of(h, kv.first));
    ts->raw.n_buckets = gen_bucket_count(h);
    if (!h->d_out_bias) {
        void* p = nullptr;
        HIP_TRY(hipMalloc(&p, 256));
        h->allocs.push_back(p);
        HIP_TRY(hipMemcpy(p, &h->out_bias, sizeof(float), hipMemcpyHostToDevice));
        h->d_out_bias = static_cast<float*>(p);
    }
    if ((rc = wgrad_setup()) != HIFICAR_OK) return rc;
    // device-resident weights only refresh the fp32 layer-by-layer packs: the fused pair kernel's packs and the bf16x3 packs would go stale
    h->use_pair = false;
    return HIFICAR_OK;
}

static void fill_pack(PackParams& pp, const ConvLayer& P, int chunk) {
    memset(&pp, 0, sizeof(pp));
    pp.n_blocks32 = P.n_blocks32;
    pp.nchunk = P.cin_pad / chunk;
    pp.ntaps = P.ntaps;
    pp.nc16 = chunk / 16;
    pp.chunk = chunk;
    pp.nb32_per_phase = P.nb32_per_phase;
    pp.total = (long long)P.n_blocks32 * pp.nchunk * P.ntaps * pp.nc16 * 2 * 256;
    pp.scale = 1.f;
    for (int r = 0; r < kMaxPhase; ++r)
        for (int t = 0; t < kMaxTaps; ++t) pp.tap_k[r][t] = (r < P.n_phase && t < P.ntaps) ? P.tap_k[r][t] : -1;
}

static int launch_pack(const PackParams& pp, hipStream_t stream) {
    const unsigned blocks = (unsigned)std::min<long long>((pp.total + 255) / 256, 2048);
    hipLaunchKernelGGL(pack_w32_kernel, dim3(blocks), dim3(256), 0, stream, pp);
    HIP_TRY(hipGetLastError());
    return HIFICAR_OK;
}

__global__ __launch_bounds__(256) static void outw_pack_kernel(const float* src, float* dst, int C, int Cp, int K) {  // (1, C, K) -> [k][Cp]
    for (int i = threadIdx.x; i < K * Cp; i += 256) {
        const int k = i / Cp, c = i - k * Cp;
        dst[i] = c < C ? src[(size_t)c * K + k] : 0.f;
    }
}

__global__ __launch_bounds__(256) static void transpose_kernel(const float* src, float* dst, int rows, int cols) {  // (rows, cols) -> (cols, rows)
    const long long n = (long long)rows * cols;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int r = (int)(i / cols), c = (int)(i - (long long)r * cols);
        dst[(size_t)c * rows + r] = src[i];
    }
}

static PackParams simple_pack(int mode, const float* src, float* dst, long long total) {
    PackParams pp;
    memset(&pp, 0, sizeof(pp));
    pp.mode = mode;
    pp.src = src;
    pp.dst = dst;
    pp.total = total;
    return pp;
}

// The device-side repacks one FOLDED parameter (reference name and layout) needs: forward pack + data-gradient pack of a conv weight,
// the bias replicated over a transposed conv's phases, the output conv's [k][Cp] layout, the PastFCEncoder's transposed matrices.
static int pack_jobs_for(hificar_handle* h, const std::string& n, const float* data, std::vector<PackParams>& jobs) {
    TrainState* ts = train_state(h);
    if (!h->weights.expected.count(n)) return fail(HIFICAR_E_INVALID, "unexpected tensor name '%s' for this configuration", n.c_str());
    const hificar_config& cfg = h->cfg;
    if (n == "output_conv.1.weight") {
        const int C = h->c_last, Cp = round_up(h->c_last, 32);
        PackParams pp = simple_pack(4, data, h->d_out_w, (long long)cfg.kernel_size * Cp);
        pp.cin = C;
        pp.cout_pad = Cp;
        pp.K = cfg.kernel_size;
        jobs.push_back(pp);
        return HIFICAR_OK;
    }
    if (n == "output_conv.1.bias") {
        jobs.push_back(simple_pack(7, data, h->d_out_bias, 1));
        return HIFICAR_OK;
    }
    if (n.rfind("ar_model.model.", 0) == 0) {
        const int l = atoi(n.c_str() + 15) / 2;
        int dims[6] = {cfg.ar_input, cfg.ar_hidden, cfg.ar_hidden, cfg.ar_hidden, cfg.ar_hidden, cfg.ar_output};
        if (n.size() >= 7 && n.compare(n.size() - 7, 7, ".weight") == 0) {
            PackParams pp = simple_pack(5, data, h->d_mlp_w[l], (long long)dims[l] * dims[l + 1]);  // (out, in) -> (in, out)
            pp.cout = dims[l + 1];
            pp.cin = dims[l];
            jobs.push_back(pp);
        } else {
            jobs.push_back(simple_pack(7, data, h->d_mlp_b[l], dims[l + 1]));
        }
        return HIFICAR_OK;
    }
    {   // speaker / phoneme conditioning (hifigan.py:176-189): plain copies into the buffers front_kernel / ph_head_kernel read
        float* dst = n == "spk_emb_mat.weight" ? h->d_spk_emb : n == "spk_fc.weight" ? h->d_spk_w : n == "spk_fc.bias" ? h->d_spk_b
                   : n == "ph_emb_mat.weight" ? h->d_ph_emb : n == "ph_fc.weight" ? h->d_phfc_w : n == "ph_fc.bias" ? h->d_phfc_b : nullptr;
        if (dst) {
            long long total = 1;
            for (auto v : h->weights.expected.at(n)) total *= v;
            jobs.push_back(simple_pack(7, data, dst, total));
            return HIFICAR_OK;
        }
    }
    const size_t dot = n.rfind('.');
    const std::string base = n.substr(0, dot), kind = n.substr(dot + 1);
    auto it = ts->by_name.find(base);
    if (it == ts->by_name.end()) return fail(HIFICAR_E_INVALID, "no conv layer '%s'", base.c_str());
    const ConvLayer& L = *it->second.first;
    const ConvLayer& D = *it->second.second;
    if (kind == "bias") {
        PackParams pp = simple_pack(6, data, L.d_bias, (long long)L.n_phase * L.cout);
        pp.cout = L.cout;
        pp.cout_pad = L.cout_pad;
        jobs.push_back(pp);
        return HIFICAR_OK;
    }
    PackParams pp;
    fill_pack(pp, L, L.chunk16);  // forward pack
    pp.src = data;
    pp.dst = L.d_w32;
    pp.mode = L.transposed ? 1 : 0;
    pp.cin = L.cin;
    pp.cout = L.cout;
    pp.K = L.K;
    pp.cin_pack = L.cin;
    pp.cout_pack = L.cout;
    jobs.push_back(pp);
    fill_pack(pp, D, D.chunk16);  // data-gradient pack
    pp.src = data;
    pp.dst = D.d_w32;
    pp.cin = L.cin;
    pp.cout = L.cout;
    pp.K = L.K;
    pp.cout_pack = L.cin;
    if (!L.transposed) {
        pp.mode = 2;
        pp.cin_pack = L.cout;
    } else {
        int stage = 0;
        for (size_t i = 0; i < h->ups.size(); ++i)
            if (&h->ups[i] == &L) stage = (int)i;
        pp.mode = 3;
        pp.cin_pack = L.cout_total;
        pp.stride = L.stride;
        pp.pad = L.padding;
        pp.cout_pad = L.cout_pad;
        pp.jmin = ts->up_jmin[stage];
        // the MRF mean in front of upsample i > 0 (hifigan.py:229: c = cs / num_blocks): its 1 / n rides on this data gradient
        pp.scale = stage > 0 ? 1.0f / (float)cfg.n_blocks : 1.0f;
    }
    jobs.push_back(pp);
    return HIFICAR_OK;
}

// One FOLDED parameter (reference name and layout, as hificar_set_weight takes it) from DEVICE memory: repacked on the device, on `stream`.
extern "C" int hificar_set_weight_device(hificar_handle* h, const char* name, const float* data, void* stream_) {
    if (!h || !name || !data) return fail(HIFICAR_E_INVALID, "hificar_set_weight_device: null argument");
    int rc = train_init(h);
    if (rc != HIFICAR_OK) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    std::vector<PackParams> jobs;
    if ((rc = pack_jobs_for(h, name, data, jobs)) != HIFICAR_OK) return rc;
    for (const PackParams& pp : jobs)
        if ((rc = launch_pack(pp, stream)) != HIFICAR_OK) return rc;
    return HIFICAR_OK;
}

template <typename T>
static int device_table(hificar_engine* h, const std::vector<T>& host, T** dev) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, std::max<size_t>(host.size(), 1) * sizeof(T)));
    h->allocs.push_back(p);
    HIP_TRY(hipMemcpy(p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    *dev = static_cast<T*>(p);
    return HIFICAR_OK;
}

// First hand-over of a raw-parameter set: the master copy, the static pack table (`packs` appends every pack of the engine, its sources
// inside r.d_folded), the job order (slots stably sorted by bucket) and the job tables with their pinned mirrors.
static int raw_setup(hificar_engine* h, RawParamSet& r, const std::function<int(std::vector<PackParams>&)>& packs) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, (size_t)r.total * sizeof(float)));
    h->allocs.push_back(p);
    r.d_folded = static_cast<float*>(p);
    std::vector<PackParams> jobs;
    int rc;
    if ((rc = packs(jobs)) != HIFICAR_OK) return rc;
    std::vector<int> start(jobs.size() + 1, 0);
    for (size_t j = 0; j < jobs.size(); ++j)
        start[j + 1] = start[j] + (int)std::max<long long>(1, std::min<long long>((jobs[j].total + 1023) / 1024, 256));
    r.n_pack_jobs = (int)jobs.size();
    r.n_pack_wgs = start.back();
    if ((rc = device_table(h, jobs, &r.d_pack_jobs)) != HIFICAR_OK) return rc;
    if ((rc = device_table(h, start, &r.d_pack_start)) != HIFICAR_OK) return rc;
    const size_t cap = r.slots.size();
    r.job_slot.resize(cap);
    for (size_t j = 0; j < cap; ++j) r.job_slot[j] = (int)j;
    std::stable_sort(r.job_slot.begin(), r.job_slot.end(), [&](int a, int b) { return r.slots[(size_t)a].bucket < r.slots[(size_t)b].bucket; });
    r.bucket_job_lo.assign((size_t)r.n_buckets + 1, (int)cap);
    for (size_t k = cap; k-- > 0;) r.bucket_job_lo[(size_t)r.slots[(size_t)r.job_slot[k]].bucket] = (int)k;
    for (int b = r.n_buckets - 1; b >= 0; --b) r.bucket_job_lo[(size_t)b] = std::min(r.bucket_job_lo[(size_t)b], r.bucket_job_lo[(size_t)b + 1]);
    HIP_TRY(hipMalloc(&p, cap * sizeof(ParamJob)));
    h->allocs.push_back(p);
    r.d_param_jobs = static_cast<ParamJob*>(p);
    HIP_TRY(hipMalloc(&p, (cap + 1) * sizeof(int)));
    h->allocs.push_back(p);
    r.d_param_start = static_cast<int*>(p);
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&r.pin_param_jobs), cap * sizeof(ParamJob), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&r.pin_param_start), (cap + 1) * sizeof(int), hipHostMallocDefault));
    return HIFICAR_OK;
}

// EVERY raw parameter of a set from device memory, in one call (two kernel launches): names[i] is a reference state_dict key —
// "<conv>.weight_g" + "<conv>.weight_v" for a weight-normed conv, "<conv>.weight" for a plain one, biases, Linear tensors.  The weight
// norm is folded on the device into the master copy, every pack is refreshed from it.  The raw-gradient buffer of
// raw_weight_norm_backward has one slot per entry, in this order, each rounded up to 4 floats.  `fn` names the entry point in messages.
static int raw_set_parameters(hificar_engine* h, RawParamSet& r, const char* fn, const char* const* names, const float* const* data, int n,
                              hipStream_t stream, const std::function<int(std::vector<PackParams>&)>& packs) {
    int rc;
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    if (!r.d_folded && (rc = raw_setup(h, r, packs)) != HIFICAR_OK) return rc;
    // raw slots in the caller's order; one job per folded slot
    std::map<std::string, int> where;
    std::vector<std::string> raw_names((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!names[i] || !data[i]) return fail(HIFICAR_E_INVALID, "%s: entry %d is null", fn, i);
        raw_names[(size_t)i] = names[i];
        if (!where.emplace(raw_names[(size_t)i], i).second) return fail(HIFICAR_E_INVALID, "%s: parameter '%s' given twice", fn, names[i]);
    }
    std::vector<ParamJob> slot_job;
    std::vector<int64_t> numel((size_t)n, -1), raw_off((size_t)n);
    std::vector<int> raw_bucket((size_t)n);
    for (const RawParamSet::Slot& s : r.slots) {
        ParamJob q;
        memset(&q, 0, sizeof(q));
        q.dst = s.offset;
        auto plain = where.find(s.name);
        auto wg = where.find(s.name + "_g"), wv = where.find(s.name + "_v");
        if (plain != where.end()) {
            q.v = data[plain->second];
            q.cols = (int)s.numel;
            q.rows = (int)((s.numel + 1023) / 1024);
            q.dv = plain->second;  // (raw index for now)
            numel[(size_t)plain->second] = s.numel;
        } else if (wg != where.end() && wv != where.end() && s.shape.size() >= 2) {
            q.v = data[wv->second];
            q.g = data[wg->second];
            q.rows = (int)s.shape[0];
            q.cols = (int)(s.numel / s.shape[0]);
            q.dv = wv->second;
            q.dg = wg->second;
            numel[(size_t)wv->second] = s.numel;
            numel[(size_t)wg->second] = s.shape[0];
            raw_bucket[(size_t)q.dg] = s.bucket;
        } else {
            return fail(HIFICAR_E_INVALID, "%s: parameter '%s' (or its weight_g / weight_v pair) is missing", fn, s.name.c_str());
        }
        raw_bucket[(size_t)q.dv] = s.bucket;
        slot_job.push_back(q);
    }
    int64_t off = 0;
    for (int i = 0; i < n; ++i) {
        if (numel[(size_t)i] < 0) return fail(HIFICAR_E_INVALID, "%s: unexpected parameter '%s'", fn, names[i]);
        raw_off[(size_t)i] = off;
        off += (numel[(size_t)i] + 3) & ~(int64_t)3;
    }
    std::vector<ParamJob> jobs(slot_job.size());  // bucket order
    for (size_t k = 0; k < jobs.size(); ++k) {
        ParamJob& q = jobs[k] = slot_job[(size_t)r.job_slot[k]];
        q.dv = raw_off[(size_t)q.dv];
        if (q.g) q.dg = raw_off[(size_t)q.dg];
    }
    r.raw_bucket = raw_bucket;
    const bool same = r.have_params && jobs.size() == r.param_jobs.size() && raw_names == r.raw_names &&
                      memcmp(jobs.data(), r.param_jobs.data(), jobs.size() * sizeof(ParamJob)) == 0;
    if (!same) {  // first call, or a parameter's storage moved: re-send the table (the pinned mirror may still be in flight)
        HIP_TRY(hipStreamSynchronize(stream));
        r.param_jobs = jobs;
        r.raw_names = raw_names;
        r.raw_total = off;
        int wgs = 0;
        for (size_t j = 0; j < jobs.size(); ++j) {
            r.pin_param_jobs[j] = jobs[j];
            r.pin_param_start[j] = wgs;
            wgs += jobs[j].rows;
        }
        r.pin_param_start[jobs.size()] = wgs;
        r.n_param_wgs = wgs;
        HIP_TRY(hipMemcpyAsync(r.d_param_jobs, r.pin_param_jobs, jobs.size() * sizeof(ParamJob), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(r.d_param_start, r.pin_param_start, (jobs.size() + 1) * sizeof(int), hipMemcpyHostToDevice, stream));
        r.have_params = true;
    }
    {
        ProfScope prof(h, stream, "param_gather_kernel", 0.0, 8.0 * r.total);
        hipLaunchKernelGGL(param_gather_kernel, dim3(r.n_param_wgs), dim3(256), 0, stream, r.d_param_jobs, r.d_param_start,
                           (int)r.param_jobs.size(), r.d_folded);
    }
    HIP_TRY(hipGetLastError());
    {
        ProfScope prof(h, stream, "pack_all_kernel", 0.0, 12.0 * r.total);
        hipLaunchKernelGGL(pack_all_kernel, dim3(r.n_pack_wgs), dim3(256), 0, stream, r.d_pack_jobs, r.d_pack_start, r.n_pack_jobs);
    }
    HIP_TRY(hipGetLastError());
    return HIFICAR_OK;
}

// Folded gradients -> gradients of the raw parameters last handed over, in that call's order (weight_g: dim-0 floats, weight_v: the
// weight's shape; every slot rounded up to 4 floats).  One launch: every job (bucket < 0), or the jobs of one bucket — meant to be called
// from the bucket callback on the stream it hands over (no cross-stream ordering is added).  grad_scale: a device scalar, or null.
// The caller checks r.have_params and the bucket's range.
static int raw_weight_norm_backward(hificar_engine* h, const RawParamSet& r, const float* grads, float* raw_grads, int bucket,
                                    const float* grad_scale, hipStream_t stream) {
    const bool all = bucket < 0;
    int rc;
    if (all && (rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    const int lo = all ? 0 : r.bucket_job_lo[(size_t)bucket], hi = all ? (int)r.param_jobs.size() : r.bucket_job_lo[(size_t)bucket + 1];
    if (!all && hi <= lo) return HIFICAR_OK;
    const int wg0 = r.pin_param_start[lo], wg1 = r.pin_param_start[hi];
    ProfScope prof(h, stream, "wn_backward_kernel", 0.0, all ? 16.0 * r.total : 0.0);
    hipLaunchKernelGGL(wn_backward_kernel, dim3(wg1 - wg0), dim3(256), 0, stream, r.d_param_jobs, r.d_param_start, (int)r.param_jobs.size(),
                       grads, raw_grads, wg0, grad_scale);
    HIP_TRY(hipGetLastError());
    return HIFICAR_OK;
}

static int raw_param_bucket(const RawParamSet* r, int i) { return r && i >= 0 && i < (int)r->raw_bucket.size() ? r->raw_bucket[(size_t)i] : -1; }

// The generator's raw parameters (hifigan.py:268-278 for the weight norm; the PastFCEncoder and the conditioning tensors included).
extern "C" int hificar_set_parameters_device(hificar_handle* h, const char* const* names, const float* const* data, int n, void* stream_) {
    if (!h || !names || !data || n < 1) return fail(HIFICAR_E_INVALID, "hificar_set_parameters_device: null argument");
    int rc = train_init(h);
    if (rc != HIFICAR_OK) return rc;
    RawParamSet& r = train_state(h)->raw;
    auto packs = [&](std::vector<PackParams>& jobs) -> int {
        for (const RawParamSet::Slot& s : r.slots)
            if ((rc = pack_jobs_for(h, s.name, r.d_folded + s.offset, jobs)) != HIFICAR_OK) return rc;
        return HIFICAR_OK;
    };
    return raw_set_parameters(h, r, "hificar_set_parameters_device", names, data, n, static_cast<hipStream_t>(stream_), packs);
}

extern "C" int64_t hificar_raw_grad_floats(const hificar_handle* h) {
    if (!h || !h->train) return -1;
    return static_cast<const TrainState*>(h->train)->raw.raw_total;
}

extern "C" int hificar_weight_norm_backward(hificar_handle* h, const float* grads, float* raw_grads, void* stream_) {
    if (!h || !grads || !raw_grads) return fail(HIFICAR_E_INVALID, "hificar_weight_norm_backward: null argument");
    TrainState* ts = train_state(h);
    if (!ts || !ts->raw.have_params) return fail(HIFICAR_E_STATE, "hificar_weight_norm_backward needs hificar_set_parameters_device first");
    return raw_weight_norm_backward(h, ts->raw, grads, raw_grads, -1, nullptr, static_cast<hipStream_t>(stream_));
}

// ---- gradient buckets (include/hificar.h: "data-parallel training") ----
extern "C" int hificar_grad_bucket_count(hificar_handle* h) {
    if (!h || train_init(h) != HIFICAR_OK) return -1;
    return gen_bucket_count(h);
}

extern "C" int hificar_raw_param_bucket(const hificar_handle* h, int i) {
    const TrainState* ts = h ? static_cast<const TrainState*>(h->train) : nullptr;
    return raw_param_bucket(ts ? &ts->raw : nullptr, i);
}

extern "C" int hificar_set_bucket_callback(hificar_handle* h, hificar_bucket_fn fn, void* user) {
    if (!h) return fail(HIFICAR_E_INVALID, "null handle");
    int rc = train_init(h);
    if (rc != HIFICAR_OK) return rc;
    train_state(h)->raw.bucket_fn = fn;
    train_state(h)->raw.bucket_user = user;
    return HIFICAR_OK;
}

extern "C" int hificar_weight_norm_backward_bucket(hificar_handle* h, const float* grads, float* raw_grads, int bucket, void* stream_) {
    if (!h || !grads || !raw_grads) return fail(HIFICAR_E_INVALID, "hificar_weight_norm_backward_bucket: null argument");
    TrainState* ts = train_state(h);
    if (!ts || !ts->raw.have_params) return fail(HIFICAR_E_STATE, "hificar_weight_norm_backward_bucket needs hificar_set_parameters_device first");
    if (bucket < 0 || bucket >= ts->raw.n_buckets) return fail(HIFICAR_E_INVALID, "bucket %d out of range", bucket);
    return raw_weight_norm_backward(h, ts->raw, grads, raw_grads, bucket, nullptr, static_cast<hipStream_t>(stream_));
}

// ------------------------------------------------------------------------------------------------
// tape / workspace plans
// ------------------------------------------------------------------------------------------------
static Tape plan_tape(const hificar_handle* h, int B, int T, void* base) {
    Tape t;
    Carver cv(base, 1024);
    const hificar_config& c = h->cfg;
    t.xin = cv.floats((size_t)B * T * h->cin_pad);
    if (h->arch == 1) {  // GBlockGenerator (hificar_gblock.hip.inc): per GBlock the two input copies at the output rate and three ReLU'd conv inputs
        t.mlp = cv.floats((size_t)B * 5 * 1024);
        size_t r = (size_t)T;
        for (size_t i = 0; i < h->gb.size(); ++i) {
            r *= (size_t)h->gb[i].scale;
            t.g_xu[i] = cv.floats<char>((size_t)B * r * h->gb[i].c1a.cin_pad);
            t.g_a1u[i] = cv.floats<char>((size_t)B * r * h->gb[i].c1a.cin_pad);
            t.g_a2[i] = cv.floats<char>((size_t)B * r * h->gb[i].c1a.cout_pad);
            t.g_a3[i] = cv.floats<char>((size_t)B * r * h->gb[i].c1a.cout_pad);
            t.g_a4[i] = cv.floats<char>((size_t)B * r * h->gb[i].c1a.cout_pad);
        }
        t.fin[0] = cv.floats((size_t)B * r * round_up(h->c_last, 32));
        t.bytes = cv.bytes();
        return t;
    }
    t.h0_s = cv.floats<char>((size_t)B * T * stage_pad(c, 0));
    t.mlp = cv.floats((size_t)B * 5 * 1024);
    size_t rows = (size_t)T;
    for (int i = 0; i < c.n_stages; ++i) {
        t.upin_s[i] = i == 0 ? t.h0_s : cv.floats<char>((size_t)B * rows * stage_pad(c, i));
        rows *= c.upsample_scales[i];
        const size_t se = (size_t)B * rows * stage_pad(c, i + 1);
        t.u_s[i] = cv.floats<char>(se);
        for (int j = 0; j < c.n_blocks; ++j)
            for (int d = 0; d < c.n_dilations[j]; ++d) {
                t.xt_s[i][j][d] = cv.floats<char>(se);
                t.x_s[i][j][d] = d + 1 < c.n_dilations[j] ? cv.floats<char>(se) : nullptr;
            }
        if (i + 1 == c.n_stages)
            for (int j = 0; j < std::max(3, c.n_blocks); ++j) t.fin[j] = cv.floats(se);
    }
    t.bytes = cv.bytes();
    return t;
}

extern "C" size_t hificar_tape_bytes(const hificar_handle* h, int B, int T) {
    if (!h || B < 1 || T < 1) return 0;
    return plan_tape(h, B, T, nullptr).bytes;
}

struct BwdWs {
    float* dx[kMaxBlk];
    float* g1[kMaxBlk];
    float* du;
    float* dm[2];
    float* dh0;
    float* dxin;
    float* partial;   // wgrad partials (largest layer)
    float* colsum;    // bias partials
    float* mlp_delta;
    float* dfeat;
    float* outp;      // output conv weight partials
    float* dspk;      // conditioning: (B, in_channels) column sums of dxin
    float* dwin;      // use_ph_loss: (B, T, Cp_last)
    float* php;       // use_ph_loss: [B * T][num_ph * (C_last + 1)] ph_fc gradient partials
    size_t partial_elems, colsum_elems, outp_elems;
    size_t bytes;
    bool accumulate;  // weight / bias gradients are ADDED to what the gradient buffer holds (hificar_disc_set_grad_accumulate)
    struct DeferredReduce* defer;  // non-null: launch_wgrad_n only collects its reductions; flush_reduce runs them all in one launch
};

// Reductions of weight / bias gradient partials waiting for one batched launch.  Each layer's partials get their own piece of the
// scratch (poff / coff advance), which a flush hands back: the launch it enqueues is ordered in front of the next layer's kernels.
struct DeferredReduce {
    std::vector<WreducePair> w;
    std::vector<int> wgx, wgy, wkind;
    std::vector<BreducePair> b;
    std::vector<int> bgx, bgy;
    size_t poff = 0, coff = 0;
    double rbytes = 0.0;
};

static constexpr size_t kReduceSlotBytes = 128 * 1024;
static constexpr size_t kReduceSlots = 48;

static int flush_reduce(hificar_engine* h, DeferredReduce& dr, hipStream_t stream) {
    if (dr.w.empty() && dr.b.empty()) {
        dr.poff = dr.coff = 0;
        return HIFICAR_OK;
    }
    // table blob: [WreducePair x nw][BreducePair x nb][wstart nw + 1][wmeta 2 nw][bstart nb + 1][bmeta nb]
    const size_t nw = dr.w.size(), nb = dr.b.size();
    const size_t o_b = nw * sizeof(WreducePair), o_ws = round_up_sz(o_b + nb * sizeof(BreducePair), 16), o_wm = o_ws + (nw + 1) * sizeof(int),
                 o_bs = o_wm + 2 * nw * sizeof(int), o_bm = o_bs + (nb + 1) * sizeof(int), bytes = round_up_sz(o_bm + nb * sizeof(int), 16);
    if (bytes > kReduceSlotBytes) return fail(HIFICAR_E_INVALID, "internal: reduction table of %zu bytes", bytes);
    std::vector<char> blob(bytes, 0);
    if (nw) memcpy(blob.data(), dr.w.data(), nw * sizeof(WreducePair));
    if (nb) memcpy(blob.data() + o_b, dr.b.data(), nb * sizeof(BreducePair));
    int* wstart = reinterpret_cast<int*>(blob.data() + o_ws);
    int* wmeta = reinterpret_cast<int*>(blob.data() + o_wm);
    int* bstart = reinterpret_cast<int*>(blob.data() + o_bs);
    int* bmeta = reinterpret_cast<int*>(blob.data() + o_bm);
    int wgs = 0;
    for (size_t j = 0; j < nw; ++j) {
        wstart[j] = wgs;
        wmeta[2 * j] = dr.wgx[j];
        wmeta[2 * j + 1] = dr.wkind[j];
        wgs += dr.wgx[j] * dr.wgy[j];
    }
    wstart[nw] = wgs;
    int bwgs = 0;
    for (size_t j = 0; j < nb; ++j) {
        bstart[j] = bwgs;
        bmeta[j] = dr.bgx[j];
        bwgs += dr.bgx[j] * dr.bgy[j];
    }
    bstart[nb] = bwgs;
    unsigned long long hash = 1469598103934665603ull;
    for (size_t i = 0; i < bytes; i += 8) {
        unsigned long long v;
        memcpy(&v, blob.data() + i, 8);
        hash = (hash ^ v) * 1099511628211ull;
    }
    hificar_engine::ReduceSlot* slot = nullptr;
    for (auto& r : h->rslots)
        if (r.hash == hash && r.bytes == bytes && memcmp(r.h, blob.data(), bytes) == 0) slot = &r;
    if (!slot) {
        if (h->rslots.size() < kReduceSlots) {
            hificar_engine::ReduceSlot r;
            void* p = nullptr;
            HIP_TRY(hipMalloc(&p, kReduceSlotBytes));
            r.d = static_cast<char*>(p);
            HIP_TRY(hipHostMalloc(&p, kReduceSlotBytes, hipHostMallocDefault));
            r.h = static_cast<char*>(p);
            HIP_TRY(hipEventCreateWithFlags(&r.ev, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&r.up, hipEventDisableTiming));
            h->rslots.push_back(r);
            slot = &h->rslots.back();
        } else {  // recycle the least recently used table once the last launch that read it has finished (long ago, normally)
            slot = &h->rslots[0];
            for (auto& r : h->rslots)
                if (r.stamp < slot->stamp) slot = &r;
            HIP_TRY(hipEventSynchronize(slot->ev));
        }
        memcpy(slot->h, blob.data(), bytes);
        slot->bytes = bytes;
        slot->hash = hash;
        HIP_TRY(hipMemcpyAsync(slot->d, slot->h, bytes, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(slot->up, stream));
        slot->up_stream = stream;
    } else if (slot->up_stream != stream) {  // a cached table first uploaded on another stream
        HIP_TRY(hipStreamWaitEvent(stream, slot->up, 0));
    }
    slot->stamp = ++h->rstamp;
    ReduceTable t;
    t.w = reinterpret_cast<const WreducePair*>(slot->d);
    t.b = reinterpret_cast<const BreducePair*>(slot->d + o_b);
    t.wstart = reinterpret_cast<const int*>(slot->d + o_ws);
    t.wmeta = reinterpret_cast<const int*>(slot->d + o_wm);
    t.bstart = reinterpret_cast<const int*>(slot->d + o_bs);
    t.bmeta = reinterpret_cast<const int*>(slot->d + o_bm);
    t.nw = (int)nw;
    t.nb = (int)nb;
    {
        std::string rname = "reduce_multi_kernel";  // with profile_detail: how many weight (w) and bias (b) reductions the launch runs
        if (h->profile_detail) rname += " w" + std::to_string(t.nw) + " b" + std::to_string(t.nb);
        ProfScope prof(h, stream, rname, 0.0, dr.rbytes);
        hipLaunchKernelGGL(reduce_multi_kernel, dim3((unsigned)(wgs + bwgs)), dim3(256), 0, stream, t);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(slot->ev, stream));
    dr = DeferredReduce();
    return HIFICAR_OK;
}

// all-taps kernel (operands staged once per chunk for every tap): up to 11 taps (one 32 x 32 accumulator per tap and wave)
static bool wgrad_all_taps(const ConvLayer& L) { return L.ntaps <= 11; }
// (more taps: the per-tap kernel, one tile of one tap per workgroup)

// one tap, at least 128 x 128 wide: the 128 x 128-tile kernel (wgrad_gemm_kernel)
static bool wgrad_gemm_form(const ConvLayer& L) { return L.ntaps == 1 && L.n_phase == 1 && L.n_blocks32 >= 4 && (L.cin_pad + 31) / 32 >= 4; }
// ... and at least 256 columns: the 128 x 256 tile (wgrad_gemm_kernel<4, 32>)
static bool wgrad_gemm_wide(const ConvLayer& L) {
    return (L.cin_pad + 31) / 32 >= 8;
}

// G rows per chunk of the all-taps kernel.  Chunks never span sequences, so sequences of at most 32 rows (the input conv and the first
// upsampler at 25 frames) take 32-row chunks instead of multiplying 39 rows of zeros; layers with at most 7 taps have too little MFMA work
// per 64-row chunk next to its barrier + staging latency (3 taps: 96 MFMAs per wave) and take 128-row chunks when the sequences are long
// enough to fill them (LDS: 2 x (32 KB + (128 + halo) x 256 B) <= 148 KB at halo 30).
static int wgrad_row_split(const ConvLayer& L);
static int wgrad_chunk_rows(const ConvLayer& L, int rows) {
    const bool can32 = wgrad_row_split(L) <= 2;  // the K loop walks 16 rows per trip: a wave's share of the chunk is at least that
    if (rows <= 32 && can32) return 32;
    if (L.ntaps <= 7 && rows > 64 && L.off_max - L.off_min <= 32) return 128;
    return 64;
}

static int wgrad_split(const hificar_engine* h, const ConvLayer& L, int nseq, int rows) {
    if (wgrad_gemm_form(L)) {
        const int aw = wgrad_gemm_wide(L) ? 8 : 4;  // 32-blocks along a per tile
        const long long tiles = (long long)((L.n_blocks32 + 3) / 4) * (((L.cin_pad + 31) / 32 + aw - 1) / aw);
        const long long nchunks = (long long)nseq * ((rows + kWggR - 1) / kWggR);
        if (tiles * 16 <= h->num_cus) return (int)std::max<long long>(1, std::min<long long>(std::min<long long>(h->num_cus / tiles, 256), nchunks));
        // few row chunks, many tiles: the split that wastes the least of the last round of workgroups (each split costs a partial pass)
        int best = 1;
        double best_cost = 1e300;
        for (int sp = 1; sp <= 16 && sp <= nchunks; ++sp) {
            const long long wgs = tiles * sp;
            const double cost = (double)((wgs + h->num_cus - 1) / h->num_cus) / sp * (1.0 + 0.02 * (sp - 1));
            if (cost < best_cost - 1e-9) {
                best_cost = cost;
                best = sp;
            }
        }
        return best;
    }
    const int gpt = (L.n_phase == 1 || L.nb32_per_phase % 2 == 0) ? 2 : 1;
    const int n_ablk = (L.cin_pad + 31) / 32;
    const bool taps = wgrad_all_taps(L);
    const long long tiles = taps ? (long long)((L.n_blocks32 + gpt - 1) / gpt) * ((n_ablk + 1) / 2)
                                 : (long long)L.ntaps * ((L.n_blocks32 + gpt - 1) / gpt) * ((n_ablk + 1) / 2);
    const int R = taps ? wgrad_chunk_rows(L, rows) : kWgR;
    const long long nchunks = (long long)nseq * ((rows + R - 1) / R);
    // workgroups ~ 2-4 per CU; the reduction reads every partial, so the split is capped (the all-taps kernel has few, fat tiles: 256)
    long long s = ((taps ? 1LL : 4LL) * h->num_cus + tiles - 1) / tiles;  // (the all-taps kernel's LDS footprint: one workgroup per CU)
    s = std::max<long long>(1, std::min<long long>(std::min<long long>(s, taps ? 256 : 32), nchunks));
    return (int)s;
}

static int wgrad_row_split(const ConvLayer& L) {
    const int gpt = (L.n_phase == 1 || L.nb32_per_phase % 2 == 0) ? 2 : 1;
    const int nblk = std::min(gpt, L.n_blocks32) * std::min(2, (L.cin_pad + 31) / 32);  // blocks the widest tile of this layer has
    return nblk >= 4 ? 1 : nblk >= 2 ? 2 : 4;
}

static size_t wgrad_partial_elems(const hificar_engine* h, const ConvLayer& L, int nseq, int rows) {
    // (room for two layers at half the split each: launch_wgrad_n)
    const size_t s2 = 2 * (size_t)std::max(1, wgrad_split(h, L, nseq, rows) / 2);
    return std::max<size_t>(s2, (size_t)wgrad_split(h, L, nseq, rows)) * L.ntaps * ((size_t)L.n_blocks32 * 32) * ((size_t)((L.cin_pad + 31) / 32) * 32);
}

// bias partials of one layer: one row of padded channels per row split (room for two layers of a paired launch, as above)
static size_t wgrad_colsum_elems(const hificar_engine* h, const ConvLayer& L, int nseq, int rows) {
    const size_t s2 = 2 * (size_t)std::max(1, wgrad_split(h, L, nseq, rows) / 2);
    return std::max<size_t>(s2, (size_t)wgrad_split(h, L, nseq, rows)) * (size_t)L.n_blocks32 * 32;
}

static constexpr int kColSplit = 64;
static constexpr int kOutSplit = 32;

static BwdWs plan_bwd(const hificar_handle* h, int B, int T, void* base) {
    BwdWs w;
    w.accumulate = false;
    w.defer = nullptr;
    Carver cv(base, 1024);
    const hificar_config& c = h->cfg;
    const size_t se = stage_elems(h, B, T);
    for (int j = 0; j < kMaxBlk; ++j) w.dx[j] = j < std::max(3, c.n_blocks) ? cv.floats(se) : nullptr;
    for (int j = 0; j < kMaxBlk; ++j) w.g1[j] = j < std::max(3, c.n_blocks) ? cv.floats(se) : nullptr;
    w.du = cv.floats(se);
    w.dm[0] = cv.floats(se);
    w.dm[1] = cv.floats(se);
    w.dh0 = cv.floats((size_t)B * T * stage_pad(c, 0));
    w.dxin = cv.floats((size_t)B * T * round_up(c.in_channels, 32));
    // weight / bias gradient partials: every layer has its own piece (the reductions of a whole pass run as ONE launch at its end, flush_reduce)
    size_t pe = wgrad_partial_elems(h, h->input_conv, B, T), ce = wgrad_colsum_elems(h, h->input_conv, B, T);
    size_t rows = (size_t)T;
    for (const GBlockLayers& g : h->gb) {  // arch 1
        rows *= (size_t)g.scale;
        for (const ConvLayer* l : {&g.c1a, &g.c1b, &g.res, &g.c2a, &g.c2b}) {
            pe += wgrad_partial_elems(h, *l, B, (int)rows);
            ce += wgrad_colsum_elems(h, *l, B, (int)rows);
        }
    }
    for (int i = 0; i < c.n_stages; ++i) {
        pe += wgrad_partial_elems(h, h->ups[i], B, (int)rows);
        ce += wgrad_colsum_elems(h, h->ups[i], B, (int)rows);
        rows *= c.upsample_scales[i];
        for (int j = 0; j < c.n_blocks; ++j)
            for (int d = 0; d < c.n_dilations[j]; ++d) {  // convs1 and convs2 of a slot have the same shape
                pe += 2 * wgrad_partial_elems(h, h->convs1[conv_index(h, i, j, d)], B, (int)rows);
                ce += 2 * wgrad_colsum_elems(h, h->convs1[conv_index(h, i, j, d)], B, (int)rows);
            }
    }
    w.partial_elems = pe;
    w.partial = cv.floats(pe);
    w.colsum_elems = ce;
    w.colsum = cv.floats(ce);
    w.mlp_delta = cv.floats((size_t)B * 5 * 512);
    w.dfeat = cv.floats((size_t)B * 512);
    w.outp_elems = (size_t)B * kOutSplit * ((size_t)c.kernel_size * round_up(h->c_last, 32) + 1);
    w.outp = cv.floats(w.outp_elems);
    w.dspk = c.use_spk_id ? cv.floats((size_t)B * c.in_channels) : nullptr;
    w.dwin = c.use_ph_loss ? cv.floats((size_t)B * T * stage_pad(c, c.n_stages)) : nullptr;
    w.php = c.use_ph_loss ? cv.floats((size_t)B * T * c.num_ph * (stage_channels(c, c.n_stages) + 1)) : nullptr;
    w.bytes = cv.bytes();
    return w;
}

extern "C" size_t hificar_backward_workspace_bytes(const hificar_handle* h, int B, int T) {
    if (!h || B < 1 || T < 1) return 0;
    return plan_bwd(h, B, T, nullptr).bytes;
}

extern "C" int hificar_grad_count(hificar_handle* h) {
    if (!h || train_init(h) != HIFICAR_OK) return -1;
    return (int)train_state(h)->raw.slots.size();
}

extern "C" int hificar_grad_info(hificar_handle* h, int i, char* name96, int64_t* offset, int64_t* numel) {
    if (!h || !name96 || !offset || !numel) return fail(HIFICAR_E_INVALID, "hificar_grad_info: null argument");
    int rc = train_init(h);
    if (rc != HIFICAR_OK) return rc;
    TrainState* ts = train_state(h);
    if (i < 0 || i >= (int)ts->raw.slots.size()) return fail(HIFICAR_E_INVALID, "gradient index %d out of range", i);
    const RawParamSet::Slot& s = ts->raw.slots[(size_t)i];
    snprintf(name96, 96, "%s", s.name.c_str());
    *offset = s.offset;
    *numel = s.numel;
    return HIFICAR_OK;
}

extern "C" int64_t hificar_grad_floats(hificar_handle* h) {
    if (!h || train_init(h) != HIFICAR_OK) return -1;
    return train_state(h)->raw.total;
}

// Forward in training mode: as hificar_forward, and every activation the backward pass needs is kept in `tape`
// (hificar_tape_bytes(h, B, T) bytes, owned by the caller until hificar_backward has run).
extern "C" int hificar_forward_train_cond(hificar_handle* h, const float* c, const float* ar, const int32_t* spk_id, const int32_t* ph, float* out,
                                          float* ph_out, int B, int T, void* workspace, size_t workspace_bytes, void* tape, size_t tape_bytes,
                                          void* stream) {
    int rc = check_ready(h, B, T, workspace, workspace_bytes);
    if (rc != HIFICAR_OK) return rc;
    if ((rc = train_init(h)) != HIFICAR_OK) return rc;
    if (h->precision != HIFICAR_PREC_F32) return fail(HIFICAR_E_INVALID, "training runs in the exact-fp32 arithmetic (precision f32)");
    if (!c || !out || !tape) return fail(HIFICAR_E_INVALID, "hificar_forward_train: null tensor");
    if (h->cfg.use_ar && !ar) return fail(HIFICAR_E_INVALID, "use_ar model needs the ar context (got NULL)");
    if (h->cfg.use_spk_id && !spk_id) return fail(HIFICAR_E_INVALID, "use_spk_id model needs spk_id (got NULL)");
    if (h->cfg.use_ph && !ph) return fail(HIFICAR_E_INVALID, "use_ph model needs ph (got NULL)");
    if (tape_bytes < plan_tape(h, B, T, nullptr).bytes || (reinterpret_cast<uintptr_t>(tape) & 255) != 0)
        return fail(HIFICAR_E_WORKSPACE, "tape too small or not 256-byte aligned: need %zu bytes", plan_tape(h, B, T, nullptr).bytes);
    if ((rc = enter_stream(h, static_cast<hipStream_t>(stream))) != HIFICAR_OK) return rc;
    const Tape tp = plan_tape(h, B, T, tape);
    FwdCall k = whole_call(h, c, ar, spk_id, ph, out, ph_out, B, T, static_cast<hipStream_t>(stream));
    k.T = T;
    k.tp = &tp;
    k.ws = plan_workspace(h, B, T, workspace);
    return forward_impl(h, k);
}

extern "C" int hificar_forward_train(hificar_handle* h, const float* c, const float* ar, float* out, int B, int T, void* workspace,
                                     size_t workspace_bytes, void* tape, size_t tape_bytes, void* stream) {
    if (h && (h->cfg.use_spk_id || h->cfg.use_ph)) return fail(HIFICAR_E_INVALID, "this model takes spk_id / ph: call hificar_forward_train_cond");
    return hificar_forward_train_cond(h, c, ar, nullptr, nullptr, out, nullptr, B, T, workspace, workspace_bytes, tape, tape_bytes, stream);
}

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
// dW (and, with db != null, the bias gradient: column sums of g taken from the staged tiles) of one conv layer
struct WgradJob {
    const ConvLayer* L;
    const float* g;
    int gpitch;
    const float* a;
    int apitch;
    float* dW;
    float* db;  // nullptr: no bias
    int gemm_cin = 0, gemm_kt = 0;  // GEMM form of a conv (discriminators): dW in the conv's (cout, gemm_cin, gemm_kt) layout
    // a grouped conv's zg groups in the same launches: group z's g / a / dW / db lie z strides (floats) further on
    int zg = 1;
    long long zs_g = 0, zs_a = 0, zs_dW = 0, zs_db = 0;
    long long a_seq_pitch = 0;  // A-operand addressing (WgradTapsParams::a_seq_pitch / acols); 0: packed rows
    int acols = 0;
    int a_rows = 0;             // A rows per sequence when they differ from `rows` (WgradTapsParams::a_rows)
    int poly_s = 0, poly_cin = 0, poly_k = 0;  // polyphase-input form of a strided conv: dW in the conv's (cout, poly_cin, poly_k) layout
    // both non-null (a wgrad_gemm_form layer, one sequence, one group): g and a as xfmr_split_rows_t_kernel wrote them, gpitch and apitch
    // channels wide; the launch is wgrad_bf16x3_kernel (the Transformer's bf16x3w training arithmetic) and g / a are not read
    const char *g16 = nullptr, *a16 = nullptr;
    // a k = 3 conv run as its one-tap GEMM twin L (the Transformer's bf16x3wac training arithmetic; with gemm_cin / gemm_kt): the conv itself,
    // whose shape the profile rows and the FLOP count carry, and the columns from one tap to the next where they are more than gemm_cin
    const ConvLayer* shape = nullptr;
    int gemm_pitch = 0;
};

// Weight (and bias) gradients of n = 1 or 2 layers over the same rows.  Two layers share one launch of each kernel when both take the
// all-taps kernel with the same tap count (conv2 + conv1 of a ResBlock slot): half the row splits each.
static int launch_wgrad_n(hificar_engine* h, const WgradJob* jobs, int n, int nseq, int rows, const BwdWs& bw, hipStream_t stream) {
    // (... and the same chunk rows: a dilated conv1 whose halo exceeds 32 rows takes 64-row chunks where its conv2 takes 128, kernel 7 at
    // dilation 6 for one; one launch has one chunk size, so such a slot runs as two launches)
    if (n == 2 && !(wgrad_all_taps(*jobs[0].L) && wgrad_all_taps(*jobs[1].L) && jobs[0].L->ntaps == jobs[1].L->ntaps &&
                    wgrad_chunk_rows(*jobs[0].L, rows) == wgrad_chunk_rows(*jobs[1].L, rows))) {
        int rc = launch_wgrad_n(h, jobs, 1, nseq, rows, bw, stream);
        return rc != HIFICAR_OK ? rc : launch_wgrad_n(h, jobs + 1, 1, nseq, rows, bw, stream);
    }
    WgradTapsPair tp;
    WreducePair rp;
    BreducePair bp;
    memset(&tp, 0, sizeof(tp));
    memset(&rp, 0, sizeof(rp));
    memset(&bp, 0, sizeof(bp));
    const int zg = jobs[0].zg;
    if (n == 2 && (zg != 1 || jobs[1].zg != 1)) return fail(HIFICAR_E_INVALID, "internal: paired weight gradients of grouped layers");
    tp.zg = rp.zg = bp.zg = zg;
    if (bw.defer) {  // deferred reductions: this call's partials go behind the pending ones; a full scratch (or table) flushes first
        size_t need_p = 0, need_c = 0;
        for (int i = 0; i < n; ++i) {
            const ConvLayer& L = *jobs[i].L;
            const size_t sp = (size_t)std::max(1, wgrad_split(h, L, nseq, rows) / (n * zg));
            need_p += sp * L.ntaps * ((size_t)L.n_blocks32 * 32) * ((size_t)((L.cin_pad + 31) / 32) * 32) * zg;
            need_c += sp * L.n_blocks32 * 32 * zg;
        }
        if (bw.defer->poff + need_p > bw.partial_elems || bw.defer->coff + need_c > bw.colsum_elems || bw.defer->w.size() >= 64) {
            int rc = flush_reduce(h, *bw.defer, stream);
            if (rc != HIFICAR_OK) return rc;
        }
        if (need_c > bw.colsum_elems) return fail(HIFICAR_E_WORKSPACE, "internal: bias partial buffer too small for %s", jobs[0].L->name.c_str());
    }
    const size_t base_p = bw.defer ? bw.defer->poff : 0, base_c = bw.defer ? bw.defer->coff : 0;
    size_t poff = 0, coff = 0, lds = 0;
    int tiles = 0, nsplit = 0;
    long long red_wgs = 0;
    double flops = 0, bytes = 0, rbytes = 0;
    bool any_bias = false;
    int bias_wgs = 0;
    const bool taps = wgrad_all_taps(*jobs[0].L);
    const bool gemm = n == 1 && wgrad_gemm_form(*jobs[0].L);
    for (int i = 0; i < n; ++i) {
        const ConvLayer& L = *jobs[i].L;
        WgradParams& wp = tp.q[i].w;
        wp.g = jobs[i].g;
        wp.a = jobs[i].a;
        wp.partial = bw.partial + base_p + poff;
        wp.nseq = nseq;
        wp.L = rows;
        wp.gpitch = jobs[i].gpitch;
        wp.apitch = jobs[i].apitch;
        wp.n_gblk = L.n_blocks32;
        wp.n_ablk = (L.cin_pad + 31) / 32;
        wp.ntaps = L.ntaps;
        wp.tap_step = L.ntaps > 1 ? L.tap_off[0][1] - L.tap_off[0][0] : 0;
        for (int r = 0; r < kMaxPhase; ++r) wp.tap_off0[r] = r < L.n_phase ? L.tap_off[r][0] : 0;
        wp.nb32_per_phase = L.nb32_per_phase;
        wp.chunks_per_seq = (rows + kWgR - 1) / kWgR;
        wp.nsplit = std::max(1, wgrad_split(h, L, nseq, rows) / (n * zg));
        wp.g_per_tile = (L.n_phase == 1 || L.nb32_per_phase % 2 == 0) ? 2 : 1;
        wp.bias_partial = jobs[i].db ? bw.colsum + base_c + coff : nullptr;
        wp.row_split = wgrad_row_split(L);
        const size_t pe = (size_t)wp.nsplit * L.ntaps * ((size_t)wp.n_gblk * 32) * ((size_t)wp.n_ablk * 32);
        if (base_p + poff + pe * zg > bw.partial_elems) return fail(HIFICAR_E_WORKSPACE, "internal: wgrad partial buffer too small for %s", L.name.c_str());
        const int t = gemm ? ((wp.n_gblk + 3) / 4) * (wgrad_gemm_wide(L) ? (wp.n_ablk + 7) / 8 : (wp.n_ablk + 3) / 4)
                           : (taps ? 1 : L.ntaps) * ((wp.n_gblk + wp.g_per_tile - 1) / wp.g_per_tile) * ((wp.n_ablk + 1) / 2);
        if (i > 0 && (t != tiles || wp.nsplit != nsplit)) return fail(HIFICAR_E_INVALID, "internal: paired weight gradients of unlike layers");
        tiles = t;
        nsplit = wp.nsplit;
        tp.q[i].zeros = h->d_zeros;
        tp.q[i].off_min = L.off_min;
        tp.q[i].halo = L.off_max - L.off_min;
        tp.q[i].a_seq_pitch = jobs[i].a_seq_pitch;
        tp.q[i].acols = jobs[i].acols;
        tp.q[i].a_rows = jobs[i].a_rows;
        tp.q[i].zs_g = jobs[i].zs_g;
        tp.q[i].zs_a = jobs[i].zs_a;
        tp.q[i].zs_partial = (long long)pe;
        tp.q[i].zs_bias = (long long)wp.nsplit * wp.n_gblk * 32;
        rp.zs_partial[i] = (long long)pe;
        rp.zs_dst[i] = jobs[i].zs_dW;
        bp.zs_partial[i] = (long long)wp.nsplit * wp.n_gblk * 32;
        bp.zs_dst[i] = jobs[i].zs_db;
        const size_t cr = (size_t)wgrad_chunk_rows(L, rows);
        lds = std::max(lds, 2 * (cr * 256 + round_up_sz((cr + tp.q[i].halo) * 256, 1024)) + 1024);  // + the K loop's over-read
        if (taps && lds > 160 * 1024)  // (a GBlock's dilation-27 conv with a kernel above 7: inference runs, its weight gradient's staging does not fit)
            return fail(HIFICAR_E_INVALID, "weight gradient of %s: %d taps reaching over %d rows need %zu KB of LDS staging (160 KB per CU); "
                        "kernels this long at this dilation run in inference only", L.name.c_str(), L.ntaps, tp.q[i].halo, lds / 1024);
        const double pos = (double)nseq * rows;
        const ConvLayer& S = jobs[i].shape ? *jobs[i].shape : L;
        flops += 2.0 * pos * S.cin * S.cout * S.K * zg;
        bytes += 4.0 * pos * (jobs[i].gpitch + jobs[i].apitch) * zg;

        WreduceParams& r = rp.r[i];
        r.partial = wp.partial;
        r.dst = jobs[i].dW;
        r.nsplit = wp.nsplit;
        r.accumulate = bw.accumulate ? 1 : 0;
        r.ntaps = L.ntaps;
        r.gpad = wp.n_gblk * 32;
        r.apad = wp.n_ablk * 32;
        r.cout = L.cout;
        r.cin = L.cin;
        r.K = L.K;
        if (jobs[i].gemm_cin > 0) {
            r.gemm_cin = jobs[i].gemm_cin;
            r.K = jobs[i].gemm_kt;
            r.gemm_pitch = jobs[i].gemm_pitch;
            r.cin = (jobs[i].gemm_pitch > 0 ? jobs[i].gemm_pitch : jobs[i].gemm_cin) * jobs[i].gemm_kt;
        }
        if (jobs[i].poly_s > 0) {
            r.poly_s = jobs[i].poly_s;
            r.poly_cin = jobs[i].poly_cin;
            r.K = jobs[i].poly_k;
        }
        r.transposed = L.transposed ? 1 : 0;
        r.n_phase = L.n_phase;
        r.cout_pad = L.cout_pad;
        for (int ph = 0; ph < kMaxPhase; ++ph)
            for (int tt = 0; tt < kMaxTaps; ++tt) r.tap_k[ph][tt] = (ph < L.n_phase && tt < L.ntaps) ? L.tap_k[ph][tt] : -1;
        const long long total = (long long)r.ntaps * r.gpad * r.apad;
        red_wgs = std::max(red_wgs, std::min<long long>((total / 4 + 255) / 256, 4096));
        rbytes += 4.0 * total * (wp.nsplit + 1);

        BreduceParams& b = bp.b[i];
        b.partial = bw.colsum + base_c + coff;
        b.dst = jobs[i].db;
        b.nsplit = wp.nsplit;
        b.pitch = wp.n_gblk * 32;
        b.cout = L.cout;
        b.cout_pad = L.cout_pad;
        b.n_phase = L.n_phase;
        b.accumulate = bw.accumulate ? 1 : 0;
        if (jobs[i].db) {
            any_bias = true;
            bias_wgs = std::max(bias_wgs, (L.cout + 15) / 16);
        }
        poff += pe * zg;
        coff += (size_t)wp.nsplit * wp.n_gblk * 32 * zg;
    }
    {
        const ConvLayer& L = *jobs[0].L;
        const ConvLayer& S = jobs[0].shape ? *jobs[0].shape : L;
        // the profile row: the kernel's name; with profile_detail the template arguments of the instantiation launched (written by the
        // macro that launches it, from the same arguments), the layer's shape and the launch's split / row split / layer count
        auto kname = [&](const char* kernel, std::initializer_list<int> targs) {
            std::string s = kernel;
            if (!h->profile_detail) return s;
            const char* sep = "<";
            for (int v : targs) {
                s += sep + std::to_string(v);
                sep = ",";
            }
            if (targs.size()) s += ">";
            return s + " " + std::to_string(S.cout) + "x" + std::to_string(S.cin) + "k" + std::to_string(S.K) + "p" + std::to_string(S.n_phase) +
                   " s" + std::to_string(nsplit) + " r" + std::to_string(tp.q[0].w.row_split) + " n" + std::to_string(n);
        };
        if (gemm && jobs[0].g16) {
            if (!jobs[0].a16 || nseq != 1 || zg != 1) return fail(HIFICAR_E_INVALID, "internal: bf16x3 weight gradient of %s", L.name.c_str());
            const WgradParams& w = tp.q[0].w;
            const WgradX3Params xp = {jobs[0].g16, jobs[0].a16, (rows + 7) / 8, w.gpitch, w.apitch, w.n_gblk, w.n_ablk, w.nsplit, w.partial, w.bias_partial, h->d_zeros};
#define HIFICAR_WGX(MI, R)                                                                                                              \
    do {                                                                                                                                \
        ProfScope prof(h, stream, kname("wgrad_bf16x3_kernel", {MI, R}), flops, bytes);                                                 \
        hipLaunchKernelGGL((wgrad_bf16x3_kernel<MI, R>), dim3(tiles, nsplit), dim3(256), (wgrad_bf16x3_lds<MI, R>()), stream, xp);      \
    } while (0)
            if (wgrad_gemm_wide(L)) HIFICAR_WGX(4, 32);
            else HIFICAR_WGX(2, 64);
#undef HIFICAR_WGX
        } else if (gemm) {
#define HIFICAR_WGG(MI, R, LDS)                                                                                            \
    do {                                                                                                                   \
        ProfScope prof(h, stream, kname("wgrad_gemm_kernel", {MI, R}), flops, bytes);                                      \
        hipLaunchKernelGGL((wgrad_gemm_kernel<MI, R>), dim3(tiles, nsplit, zg), dim3(256), LDS, stream, tp);               \
    } while (0)
            if (wgrad_gemm_wide(L)) HIFICAR_WGG(4, 32, 2 * 32 * 384 * sizeof(float) + 2048);
            else HIFICAR_WGG(2, 64, 4 * kWggR * 128 * sizeof(float) + 1024);
#undef HIFICAR_WGG
        } else if (taps) {
            const dim3 grid(tiles, nsplit, n * zg);
            const int cr = wgrad_chunk_rows(L, rows);
            if (n == 2 && wgrad_chunk_rows(*jobs[1].L, rows) != cr) return fail(HIFICAR_E_INVALID, "internal: paired weight gradients with unlike chunks");
#define HIFICAR_WGT1(NT, EX, R)                                                                                    \
    do {                                                                                                           \
        ProfScope prof(h, stream, kname("wgrad_taps_kernel", {NT, EX, R}), flops, bytes);                          \
        hipLaunchKernelGGL((wgrad_taps_kernel<NT, EX, R>), grid, dim3(256), lds, stream, tp);                      \
    } while (0)
#define HIFICAR_WGT(NT, EX)                                                                                        \
    do {                                                                                                           \
        if (cr == 32) HIFICAR_WGT1(NT, EX, 32);                                                                    \
        else if (cr == 128) HIFICAR_WGT1((NT <= 7 ? NT : 7), EX, 128);                                             \
        else HIFICAR_WGT1(NT, EX, 64);                                                                             \
    } while (0)
            switch (L.ntaps) {
                case 1: HIFICAR_WGT(1, true); break;
                case 2: HIFICAR_WGT(2, true); break;
                case 3: HIFICAR_WGT(3, true); break;
                case 7: HIFICAR_WGT(7, true); break;
                case 11: HIFICAR_WGT(11, true); break;
                default:
                    if (L.ntaps < 7) HIFICAR_WGT(7, false);
                    else HIFICAR_WGT(11, false);
            }
#undef HIFICAR_WGT
#undef HIFICAR_WGT1
        } else {
            if (zg != 1) return fail(HIFICAR_E_INVALID, "internal: grouped weight gradients need the all-taps kernel");
            ProfScope prof(h, stream, kname("wgrad_kernel", {}), flops, bytes);
            hipLaunchKernelGGL(wgrad_kernel, dim3(tiles, nsplit), dim3(256), 0, stream, tp.q[0].w);
        }
    }
    HIP_TRY(hipGetLastError());
    // GEMM form with 3 or 5 taps, gradient rows that start on 16-byte boundaries, and enough (g, 4 c) units to fill the chip (a thread
    // walks all the splits of all its taps one after the other: the small layers with hundreds of splits stay on the generic kernel,
    // measured 3 x slower here): the contiguous-store kernel
    const WreduceParams& r0 = rp.r[0];
    const bool contiguous = n == 1 && r0.gemm_cin > 0 && r0.gemm_pitch == 0 && r0.gemm_cin % 4 == 0 && (r0.K == 3 || r0.K == 5) && r0.ntaps == 1 &&
                            (long long)r0.cout * (r0.gemm_cin / 4) * zg >= 64LL * 1024 &&
                            (reinterpret_cast<uintptr_t>(r0.dst) & 15) == 0 && (rp.zs_dst[0] & 3) == 0 && (rp.zs_partial[0] & 3) == 0;
    const long long gemm_units = (long long)r0.cout * (r0.gemm_cin / 4);
    if (bw.defer) {
        DeferredReduce& dr = *bw.defer;
        dr.w.push_back(rp);
        dr.wgx.push_back(contiguous ? (int)std::min<long long>((gemm_units + 255) / 256, 4096) : (int)red_wgs);
        dr.wgy.push_back(contiguous ? zg : n * zg);
        dr.wkind.push_back(contiguous ? r0.K : 0);
        if (any_bias) {
            dr.b.push_back(bp);
            dr.bgx.push_back(bias_wgs);
            dr.bgy.push_back(n * zg);
        }
        dr.poff += poff;
        dr.coff += coff;
        dr.rbytes += rbytes;
        return HIFICAR_OK;
    }
    {
        const int gemm_k = r0.K == 5 ? 5 : 3;  // the contiguous kernel's instantiation
        std::string rname = "wreduce_kernel";
        if (h->profile_detail) {
            const ConvLayer& L = jobs[0].shape ? *jobs[0].shape : *jobs[0].L;
            if (contiguous) rname = "wreduce_gemm_kernel<" + std::to_string(gemm_k) + ">";
            rname += " " + std::to_string(L.cout) + "x" + std::to_string(L.cin) + "k" + std::to_string(L.K) + " s" + std::to_string(nsplit) + " n" + std::to_string(n) + " z" + std::to_string(zg);
        }
        ProfScope prof(h, stream, rname, 0.0, rbytes);
        if (contiguous) {
            const dim3 grid((unsigned)std::min<long long>((gemm_units + 255) / 256, 4096), zg);
            if (gemm_k == 5) hipLaunchKernelGGL(wreduce_gemm_kernel<5>, grid, dim3(256), 0, stream, rp);
            else hipLaunchKernelGGL(wreduce_gemm_kernel<3>, grid, dim3(256), 0, stream, rp);
        } else {
            hipLaunchKernelGGL(wreduce_kernel, dim3((unsigned)red_wgs, n * zg), dim3(256), 0, stream, rp);
        }
    }
    HIP_TRY(hipGetLastError());
    if (any_bias) {
        hipLaunchKernelGGL(breduce_kernel, dim3(bias_wgs, n * zg), dim3(256), 0, stream, bp);
        HIP_TRY(hipGetLastError());
    }
    return HIFICAR_OK;
}

static int launch_wgrad(hificar_engine* h, const ConvLayer& L, const float* g, int gpitch, const float* a, int apitch, int nseq, int rows,
                        float* dW, const BwdWs& bw, hipStream_t stream, float* db = nullptr) {
    const WgradJob job = {&L, g, gpitch, a, apitch, dW, db};
    return launch_wgrad_n(h, &job, 1, nseq, rows, bw, stream);
}

// Output conv + tanh backwards (hifigan.py:146-159 / gblock_gen.py:71-93): -> bw.dm[0] = gradient of each of the `nin` averaged inputs, and the
// output conv's weight / bias gradients
static int bwd_output_conv(hificar_handle* h, TrainState* ts, const Tape& tp, const BwdWs& bw, const float* dout, const float* out, int B, int T, int rows,
                           int nin, float* grads, hipStream_t stream) {
    const hificar_config& cfg = h->cfg;
    auto G = [&](const std::string& name) { return grads + ts->raw.offset(name); };
        OutBwdParams op;
        memset(&op, 0, sizeof(op));
        fill_inputs(op, tp.fin, nin);
        op.w = h->d_out_w;
        op.dout = dout;
        op.out = out;
        op.io_bstride = (int64_t)h->hop * T;
        op.dm = bw.dm[0];
        op.partial = bw.outp;
        op.L = rows;
        op.Cp = round_up(h->c_last, 32);
        op.K = cfg.kernel_size;
        op.slope = 0.01f;
        op.use_tanh = cfg.use_tanh;
        const long long units = (long long)rows * (op.Cp / 4);
        {
            ProfScope prof(h, stream, "outconv_bwd_data_kernel", 2.0 * B * rows * op.Cp * op.K, 4.0 * B * (double)rows * op.Cp * (nin + 1));
            hipLaunchKernelGGL(outconv_bwd_data_kernel, dim3((unsigned)std::min<long long>((units + 255) / 256, 1024), B), dim3(256), 0, stream, op);
        }
        HIP_TRY(hipGetLastError());
        const int rows_per = (rows + kOutSplit - 1) / kOutSplit;
        {
            ProfScope prof(h, stream, "outconv_bwd_weight_kernel", 2.0 * B * rows * op.Cp * op.K, 4.0 * B * (double)rows * op.Cp * nin);
            hipLaunchKernelGGL(outconv_bwd_weight_kernel, dim3(kOutSplit, B), dim3(256), (size_t)rows_per * sizeof(float), stream, op);
        }
        HIP_TRY(hipGetLastError());
        VreduceParams vp;
        memset(&vp, 0, sizeof(vp));
        vp.partial = bw.outp;
        vp.n = B * kOutSplit;
        vp.stride = op.K * op.Cp + 1;
        vp.len = op.K * op.Cp;
        vp.dst = G("output_conv.1.weight");
        vp.tr_K = op.K;
        vp.tr_C = h->c_last;
        vp.tr_Cp = op.Cp;
        hipLaunchKernelGGL(vreduce_kernel, dim3((vp.len + 15) / 16), dim3(256), 0, stream, vp);
        vp.partial = bw.outp + op.K * op.Cp;
        vp.len = 1;
        vp.dst = G("output_conv.1.bias");
        vp.tr_K = 0;
        hipLaunchKernelGGL(vreduce_kernel, dim3(1), dim3(256), 0, stream, vp);
        HIP_TRY(hipGetLastError());
    return HIFICAR_OK;
}

// The front of either generator backwards: input conv (weight / bias gradients from dh0 = the gradient of its output; its data gradient -> dc,
// the PastFCEncoder's output gradient, the speaker / phoneme tensors), then the PastFCEncoder
static int bwd_front(hificar_handle* h, TrainState* ts, const Tape& tp, const BwdWs& bw, float* grads, float* dc, float* dar, const int32_t* spk_id,
                     const int32_t* ph, int B, int T, hipStream_t stream) {
    const hificar_config& cfg = h->cfg;
    auto G = [&](const std::string& name) { return grads + ts->raw.offset(name); };
    const float slope = cfg.lrelu_slope;
    Ragged rg;  // dense
    rg.frames = T;
    int rc;
    // ---- input conv (no activation in front of it) ----
    {
        const ConvLayer& I = h->input_conv;
        if ((rc = launch_wgrad(h, I, bw.dh0, I.cout_total, tp.xin, I.cin_pad, B, T, G("input_conv.weight"), bw, stream, G("input_conv.bias"))) != HIFICAR_OK)
            return rc;
        if (dc || dar || cfg.use_ar || cfg.use_spk_id || cfg.use_ph) {
            const ConvLayer* lay[1] = {&ts->dg_input};
            const ConvIO io[1] = {{reinterpret_cast<const char*>(bw.dh0), nullptr, bw.dxin, nullptr}};
            if ((rc = launch_conv(h, lay, 1, B, T, io, slope, rg, stream)) != HIFICAR_OK) return rc;
            XinGradParams xp;
            xp.dxin = bw.dxin;
            xp.dc = dc;
            xp.dfeat = cfg.use_ar ? bw.dfeat : nullptr;
            xp.T = T;
            xp.cf = h->cf;
            xp.ar_out = cfg.use_ar ? cfg.ar_output : 0;
            xp.cin_pad = ts->dg_input.cout_total;
            hipLaunchKernelGGL(xin_grad_kernel, dim3(B), dim3(256), 0, stream, xp);
            HIP_TRY(hipGetLastError());
            if (cfg.use_spk_id || cfg.use_ph) {  // speaker vector / phoneme embeddings (hifigan.py:212-220)
                CondBwdParams cp;
                memset(&cp, 0, sizeof(cp));
                cp.dxin = bw.dxin;
                cp.B = B;
                cp.T = T;
                cp.cin_pad = ts->dg_input.cout_total;
                if (cfg.use_spk_id) {
                    cp.spk_id = spk_id;
                    cp.spk_emb = h->d_spk_emb;
                    cp.spk_w = h->d_spk_w;
                    cp.spk_e = cfg.spk_emb_size;
                    cp.ch = cfg.in_channels;  // (use_spk_id excludes use_ph: every input channel gets the speaker vector)
                    cp.num_spk = cfg.num_spk;
                    cp.dspk = bw.dspk;
                    cp.d_spk_emb = G("spk_emb_mat.weight");
                    cp.d_spk_w = G("spk_fc.weight");
                    cp.d_spk_b = G("spk_fc.bias");
                    hipLaunchKernelGGL(cond_spk_colsum_kernel, dim3(B), dim3(256), 0, stream, cp);
                    hipLaunchKernelGGL(cond_spk_bwd_kernel, dim3((cp.ch + 255) / 256 + (cp.num_spk * cp.spk_e + 255) / 256), dim3(256), 0, stream, cp);
                }
                if (cfg.use_ph) {
                    cp.ph = ph;
                    cp.ph_e = cfg.ph_emb_size;
                    cp.ph_off = h->cf + (cfg.use_ar ? cfg.ar_output : 0);
                    cp.num_ph = cfg.num_ph;
                    cp.d_ph_emb = G("ph_emb_mat.weight");
                    hipLaunchKernelGGL(cond_ph_emb_bwd_kernel, dim3(cfg.num_ph), dim3(256), 0, stream, cp);
                }
                HIP_TRY(hipGetLastError());
            }
        }
    }
    // ---- PastFCEncoder ----
    if (cfg.use_ar) {
        MlpBwdParams mp;
        memset(&mp, 0, sizeof(mp));
        mp.h = tp.mlp;
        mp.dfeat = bw.dfeat;
        mp.delta = bw.mlp_delta;
        mp.dar = dar;
        int dims[6] = {cfg.ar_input, cfg.ar_hidden, cfg.ar_hidden, cfg.ar_hidden, cfg.ar_hidden, cfg.ar_output};
        for (int l = 0; l < 6; ++l) mp.dims[l] = dims[l];
        for (int l = 0; l < 5; ++l) {
            mp.wt[l] = h->d_mlp_w[l];
            mp.dW[l] = G("ar_model.model." + std::to_string(2 * l) + ".weight");
            mp.db[l] = G("ar_model.model." + std::to_string(2 * l) + ".bias");
        }
        mp.B = B;
        hipLaunchKernelGGL(mlp_bwd_delta_kernel, dim3(B), dim3(256), 0, stream, mp);
        hipLaunchKernelGGL(mlp_bwd_weight_kernel, dim3(64, 5), dim3(256), 0, stream, mp);
        HIP_TRY(hipGetLastError());
    }
    return HIFICAR_OK;
}

static int gblock_backward(hificar_handle* h, TrainState* ts, const Tape& tp, BwdWs& bw, struct DeferredReduce& pending, const float* dout,
                           const float* out, const int32_t* spk_id, int B, int T, float* grads, float* dc, float* dar, hipStream_t stream);

// Gradients of one forward_train.  dout: (B, hop*T) gradient of the waveform; out: the waveform that forward returned; tape: its tape.
// grads: device buffer of hificar_grad_floats(h) floats, receives every folded parameter's gradient at its hificar_grad_info offset.
// dc: (B, cf, T) gradient of the features or NULL; dar: (B, ar_input) gradient of the AR context or NULL.
extern "C" int hificar_backward_cond(hificar_handle* h, const float* dout, const float* dph_out, const float* out, const int32_t* spk_id,
                                     const int32_t* ph, int B, int T, const void* tape, size_t tape_bytes, float* grads, float* dc, float* dar,
                                     void* workspace, size_t workspace_bytes, void* stream_) {
    if (!h || !dout || !out || !tape || !grads || !workspace) return fail(HIFICAR_E_INVALID, "hificar_backward: null argument");
    if (h->cfg.use_spk_id && !spk_id) return fail(HIFICAR_E_INVALID, "use_spk_id model: the backward pass needs spk_id again (got NULL)");
    if (h->cfg.use_ph && !ph) return fail(HIFICAR_E_INVALID, "use_ph model: the backward pass needs ph again (got NULL)");
    int rc = train_init(h);
    if (rc != HIFICAR_OK) return rc;
    if (h->precision != HIFICAR_PREC_F32) return fail(HIFICAR_E_INVALID, "training runs in the exact-fp32 arithmetic (precision f32)");
    if (B < 1 || T < 1) return fail(HIFICAR_E_INVALID, "B=%d, T=%d must be positive", B, T);
    if (tape_bytes < plan_tape(h, B, T, nullptr).bytes) return fail(HIFICAR_E_WORKSPACE, "tape too small");
    if (workspace_bytes < plan_bwd(h, B, T, nullptr).bytes || (reinterpret_cast<uintptr_t>(workspace) & 255) != 0)
        return fail(HIFICAR_E_WORKSPACE, "backward workspace too small or misaligned: need %zu bytes", plan_bwd(h, B, T, nullptr).bytes);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = enter_stream(h, stream)) != HIFICAR_OK) return rc;
    TrainState* ts = train_state(h);
    const hificar_config& cfg = h->cfg;
    const Tape tp = plan_tape(h, B, T, const_cast<void*>(tape));
    BwdWs bw = plan_bwd(h, B, T, workspace);
    DeferredReduce pending;  // the weight / bias gradient reductions wait for one launch per gradient bucket (without a callback: one per pass)
    bw.defer = &pending;
    if (h->arch == 1) return gblock_backward(h, ts, tp, bw, pending, dout, out, spk_id, B, T, grads, dc, dar, stream);
    const int nbk = cfg.n_blocks;
    const float slope = cfg.lrelu_slope;
    auto G = [&](const std::string& name) { return grads + ts->raw.offset(name); };
    Ragged rg;  // dense
    rg.frames = T;
    const BlockOrder bo = block_order(cfg);
    const bool add_convs = cfg.use_additional_convs != 0;

    int rows = T * h->hop;
    if ((rc = bwd_output_conv(h, ts, tp, bw, dout, out, B, T, rows, nbk, grads, stream)) != HIFICAR_OK) return rc;
    // ---- phoneme-loss head (hifigan.py:232-237): its gradient joins the output conv's on the last stage's ResBlock outputs ----
    if (cfg.use_ph_loss) {
        const int C = stage_channels(cfg, cfg.n_stages);
        if (dph_out) {
            PhHeadBwdParams pq;
            memset(&pq, 0, sizeof(pq));
            fill_inputs(pq, tp.fin, nbk);
            pq.w = h->d_phfc_w;
            pq.dph_out = dph_out;
            pq.dwin = bw.dwin;
            pq.partial = bw.php;
            pq.dm = bw.dm[0];
            pq.C = C;
            pq.Cp = stage_pad(cfg, cfg.n_stages);
            pq.L = rows;
            pq.T = T;
            pq.hop = h->hop;
            pq.num_ph = cfg.num_ph;
            {
                ProfScope prof(h, stream, "ph_head_bwd_kernel", 4.0 * B * T * (double)C * cfg.num_ph, 4.0 * B * (double)rows * pq.Cp * nbk);
                hipLaunchKernelGGL(ph_head_bwd_kernel, dim3(T, B), dim3(256), 0, stream, pq);
            }
            const long long units = (long long)rows * (pq.Cp / 4);
            hipLaunchKernelGGL(ph_dm_add_kernel, dim3((unsigned)std::min<long long>((units + 255) / 256, 1024), B), dim3(256), 0, stream, pq);
            HIP_TRY(hipGetLastError());
            VreduceParams vp;
            memset(&vp, 0, sizeof(vp));
            vp.partial = bw.php;
            vp.n = B * T;
            vp.stride = cfg.num_ph * (C + 1);
            vp.len = cfg.num_ph * C;
            vp.dst = G("ph_fc.weight");
            hipLaunchKernelGGL(vreduce_kernel, dim3((vp.len + 15) / 16), dim3(256), 0, stream, vp);
            vp.partial = bw.php + (size_t)cfg.num_ph * C;
            vp.len = cfg.num_ph;
            vp.dst = G("ph_fc.bias");
            hipLaunchKernelGGL(vreduce_kernel, dim3((vp.len + 15) / 16), dim3(256), 0, stream, vp);
            HIP_TRY(hipGetLastError());
        } else {  // ph_out took no part in the loss
            HIP_TRY(hipMemsetAsync(G("ph_fc.weight"), 0, (size_t)cfg.num_ph * C * sizeof(float), stream));
            HIP_TRY(hipMemsetAsync(G("ph_fc.bias"), 0, (size_t)cfg.num_ph * sizeof(float), stream));
        }
    }
    // ---- stages, last to first ----
    int dmi = 0;  // bw.dm[dmi]: gradient of each ResBlock output of the current stage
    for (int i = cfg.n_stages - 1; i >= 0; --i) {
        const int Cp = stage_pad(cfg, i + 1);
        const float* dsrc[kMaxBlk] = {bw.dm[dmi], bw.dm[dmi], bw.dm[dmi], bw.dm[dmi]};
        for (int d = bo.max_d - 1; d >= 0; --d) {
            const ConvLayer* f1[kMaxBlk];
            const ConvLayer* f2[kMaxBlk];
            const ConvLayer* d1[kMaxBlk];
            const ConvLayer* d2[kMaxBlk];
            ConvIO io2[kMaxBlk], io1[kMaxBlk];
            float* dst1[kMaxBlk];
            const Branches br = gather_branches(h, bo, i, d);
            for (int n = 0; n < br.n; ++n) {
                const int j = br.j[n], ci = br.ci[n];
                f1[n] = &h->convs1[ci];
                d1[n] = &ts->dg_c1[ci];
                const float* a1 = reinterpret_cast<const float*>(d == 0 ? tp.u_s[i] : tp.x_s[i][j][d - 1]);
                if (add_convs) {
                    f2[n] = &h->convs2[ci];
                    d2[n] = &ts->dg_c2[ci];
                    const float* a2 = reinterpret_cast<const float*>(tp.xt_s[i][j][d]);
                    io2[n] = {reinterpret_cast<const char*>(dsrc[j]), nullptr, bw.g1[j], nullptr, a2, slope};           // g1 = act'(a2) * dgrad2
                    io1[n] = {reinterpret_cast<const char*>(bw.g1[j]), dsrc[j], bw.dx[j], nullptr, a1, slope};           // dx = skip + act'(a1) * dgrad1
                    dst1[n] = bw.dx[j];
                } else {
                    // x = x + conv1(LeakyReLU(x)): dx = skip + act'(a1) * dgrad1(dy), written to the buffer the gradient is NOT read from (halo rows)
                    f2[n] = nullptr;
                    d2[n] = nullptr;
                    dst1[n] = dsrc[j] == bw.dx[j] ? bw.g1[j] : bw.dx[j];
                    io1[n] = {reinterpret_cast<const char*>(dsrc[j]), dsrc[j], dst1[n], nullptr, a1, slope};
                }
            }
            if (br.n == 0) continue;
            if (add_convs && (rc = launch_n(h, d2, nullptr, br.n, B, rows, io2, nullptr, slope, rg, stream)) != HIFICAR_OK) return rc;
            for (int q = 0; q < br.n; ++q) {
                // weight / bias gradients of the slot's two convs in one launch: conv2 from (its input a2, the gradient of its output =
                // the running skip gradient), conv1 from (its input a1, g1)
                const int j = br.j[q];
                const float* a1 = reinterpret_cast<const float*>(d == 0 ? tp.u_s[i] : tp.x_s[i][j][d - 1]);
                if (!add_convs) {  // one conv per layer: its weight gradient from (a1, the running gradient)
                    const WgradJob one[1] = {{f1[q], dsrc[j], Cp, a1, Cp, G(f1[q]->name + ".weight"), f1[q]->has_bias ? G(f1[q]->name + ".bias") : nullptr}};
                    if ((rc = launch_wgrad_n(h, one, 1, B, rows, bw, stream)) != HIFICAR_OK) return rc;
                    continue;
                }
                const float* a2 = reinterpret_cast<const float*>(tp.xt_s[i][j][d]);
                const WgradJob pairj[2] = {
                    {f2[q], dsrc[j], Cp, a2, Cp, G(f2[q]->name + ".weight"), f2[q]->has_bias ? G(f2[q]->name + ".bias") : nullptr},
                    {f1[q], bw.g1[j], Cp, a1, Cp, G(f1[q]->name + ".weight"), f1[q]->has_bias ? G(f1[q]->name + ".bias") : nullptr}};
                if ((rc = launch_wgrad_n(h, pairj, 2, B, rows, bw, stream)) != HIFICAR_OK) return rc;
            }
            if ((rc = launch_n(h, d1, nullptr, br.n, B, rows, io1, nullptr, slope, rg, stream)) != HIFICAR_OK) return rc;
            for (int q = 0; q < br.n; ++q) dsrc[br.j[q]] = dst1[q];
        }
        // every ResBlock gradient of stage i (and, for the last stage, the output conv's and the phoneme head's) is enqueued: bucket done
        if (ts->raw.bucket_fn) {
            if ((rc = flush_reduce(h, pending, stream)) != HIFICAR_OK) return rc;
            ts->raw.bucket_fn(cfg.n_stages - 1 - i, stream, ts->raw.bucket_user);
        }
        // gradient of the upsample output: the sum over the ResBlocks
        {
            const long long n4 = (long long)B * rows * Cp / 4;
            ProfScope prof(h, stream, "add3_kernel", 0.0, 16.0 * n4 * (nbk + 1));
            hipLaunchKernelGGL(add3_kernel, dim3((unsigned)std::min<long long>((n4 + 255) / 256, 8LL * h->num_cus)), dim3(256), 0, stream, dsrc[0],
                               nbk > 1 ? dsrc[1] : nullptr, nbk > 2 ? dsrc[2] : nullptr, nbk > 3 ? dsrc[3] : nullptr, bw.du, n4, nbk);
        }
        HIP_TRY(hipGetLastError());
        // upsample i: rows_in virtual rows of s * Cout_pad channels are the same memory as rows real rows of Cout_pad channels
        const ConvLayer& U = h->ups[i];
        const int rows_in = rows / cfg.upsample_scales[i];
        const float* a_up = reinterpret_cast<const float*>(tp.upin_s[i]);
        if ((rc = launch_wgrad(h, U, bw.du, U.cout_total, a_up, U.cin_pad, B, rows_in, G(U.name + ".weight"), bw, stream, G(U.name + ".bias"))) != HIFICAR_OK)
            return rc;
        {
            const ConvLayer* lay[1] = {&ts->dg_ups[i]};
            float* dst = i > 0 ? bw.dm[dmi ^ 1] : bw.dh0;
            const ConvIO io[1] = {{reinterpret_cast<const char*>(bw.du), nullptr, dst, nullptr, a_up, slope}};
            if ((rc = launch_conv(h, lay, 1, B, rows_in, io, slope, rg, stream)) != HIFICAR_OK) return rc;
        }
        dmi ^= 1;
        rows = rows_in;
    }
    if ((rc = bwd_front(h, ts, tp, bw, grads, dc, dar, spk_id, ph, B, T, stream)) != HIFICAR_OK) return rc;
    if ((rc = flush_reduce(h, pending, stream)) != HIFICAR_OK) return rc;
    if (ts->raw.bucket_fn) ts->raw.bucket_fn(cfg.n_stages, stream, ts->raw.bucket_user);  // the "front" bucket: everything else
    return HIFICAR_OK;
}

extern "C" int hificar_backward(hificar_handle* h, const float* dout, const float* out, int B, int T, const void* tape, size_t tape_bytes,
                                float* grads, float* dc, float* dar, void* workspace, size_t workspace_bytes, void* stream) {
    if (h && (h->cfg.use_spk_id || h->cfg.use_ph)) return fail(HIFICAR_E_INVALID, "this model takes spk_id / ph: call hificar_backward_cond");
    return hificar_backward_cond(h, dout, nullptr, out, nullptr, nullptr, B, T, tape, tape_bytes, grads, dc, dar, workspace, workspace_bytes, stream);
}
